"""Round-trip evaluation: encode -> VQ -> decode a set of clips in ragged batches and report the quality metrics of
metrics.RoundTripMetrics (inference_full.py:700-737's validation loop without the host copies; STOI with --stoi,
DESIGN.md §21; PESQ is not computed).

    python -m audiotokenization_amd.evaluate --save_path RUN --subsets test-clean --stoi --json OUT.json
"""
from __future__ import annotations

import json
import os
from typing import List, Optional

import torch

from .codec import _refuse_ragged
from .extract import READ_AHEAD, BigCodecModel, build_lm, find_items, item_path, plan_batches, whole_clips_only
from .metrics import RoundTripMetrics


def _as_model(model) -> BigCodecModel:
    """A BigCodecModel that reconstructs, from one or from a CodecLightningModule."""
    if isinstance(model, BigCodecModel):
        return model if model.reconstruct else BigCodecModel(model.lm, reconstruct=True)
    return BigCodecModel(model, reconstruct=True)


def _ragged_ok(lm) -> bool:
    """Whether the model takes ragged batches (antialias / a bidirectional ResLSTM / the Conformer-STFT family refuse
    them: file by file then)."""
    if whole_clips_only(lm):
        return False
    try:
        _refuse_ragged(lm.model["CodecEnc"])
        _refuse_ragged(lm.model["generator"])
    except NotImplementedError:
        return False
    return True


def _load(item, sample_rate, duration, device) -> torch.Tensor:
    """One clip as a (1, T) float32 device tensor: a path (ingest.load_item: decode, trim / pad, resample; the first
    channel) or a (T,) / (1, T) tensor."""
    if isinstance(item, (str, os.PathLike)):
        from .ingest import load_item

        wav, _ = load_item(os.fspath(item), sample_rate, duration, None, device)
        return wav[:1].float()
    t = torch.as_tensor(item)
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[0] != 1:
        raise ValueError(f"evaluate_round_trip: a clip is a path or a (T,) / (1, T) tensor, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32)


def evaluate_round_trip(model, clips_or_paths, batch: int = 16, sample_rate: Optional[int] = None,
                        duration: Optional[float] = None, device=None, per_file: bool = False,
                        metrics: Optional[RoundTripMetrics] = None, stoi: bool = False,
                        stoi_clean: str = "ref") -> dict:
    """Round-trip every clip through `model` (a CodecLightningModule or an extract.BigCodecModel) and return
    RoundTripMetrics.compute()'s dict; per_file adds "files": one {"index", "path", "samples", "si_snr",
    "mel_distance"} row per clip (a host copy per batch).  Clips are grouped by length (extract.plan_batches) into
    ragged batches of at most `batch`, both signals are cut to each clip's own length (the shorter of the clip and
    its reconstruction), and a model that refuses ragged batches runs clip by clip.  sample_rate: the rate files are
    resampled to and the mel scale's (default 16000).  stoi adds "stoi" and "stoi_short_clips" (and "stoi" to the
    rows); stoi_clean: "ref" scores the reconstruction against the input, "rec" swaps them as inference_full.py:724
    does (both ignored when `metrics` is given: that object's own settings hold)."""
    if batch < 1:
        raise ValueError("batch must be >= 1")
    m = _as_model(model)
    lm = m.lm
    enc, dec = lm.model["CodecEnc"], lm.model["generator"]
    device = torch.device(device) if device is not None else next(enc.parameters()).device
    rate = int(sample_rate) if sample_rate else 16000
    if metrics is None:
        metrics = RoundTripMetrics(rate, m.codebook_size, stoi=stoi, stoi_clean=stoi_clean)
    if not _ragged_ok(lm):
        batch = 1
    items = list(clips_or_paths)
    rows: List[dict] = []
    window = READ_AHEAD * batch
    for w0 in range(0, len(items), window):
        wavs = [_load(it, sample_rate, duration, device) for it in items[w0:w0 + window]]
        for group in plan_batches([int(w.shape[1]) for w in wavs], batch, window=max(1, len(wavs))):
            lens = [int(wavs[j].shape[1]) for j in group]
            x = torch.zeros((len(group), 1, max(lens)), device=device, dtype=torch.float32)
            for b, j in enumerate(group):
                x[b, :, :lens[b]] = wavs[j]
            with torch.no_grad():
                if len(group) == 1:
                    out = m(x)
                    frames = [int(out["indices"].shape[-1])]
                    rec_lens = [int(out["x_rec"].shape[-1])]
                else:
                    out = m(x, lengths=lens)
                    frames = [int(f) for f in out["frames"]]
                    rec_lens = dec.sample_lengths(frames)
                rec = out["x_rec"]
                Tm = min(x.shape[-1], rec.shape[-1])
                own = [min(a, b) for a, b in zip(lens, rec_lens)]
                metrics.update(x[..., :Tm], rec[..., :Tm], lengths=own, codes=out["indices"], frame_lengths=frames)
            if per_file:
                pc = metrics.per_clip()
                snr, mel = pc["si_snr"].cpu().tolist(), pc["mel_distance"].cpu().tolist()
                sto = pc["stoi"].cpu().tolist() if "stoi" in pc else None
                for b, j in enumerate(group):
                    it = items[w0 + j]
                    rows.append({"index": w0 + j, "path": os.fspath(it) if isinstance(it, (str, os.PathLike)) else None,
                                 "samples": own[b], "si_snr": snr[b], "mel_distance": mel[b]})
                    if sto is not None:
                        rows[-1]["stoi"] = sto[b]
    result = metrics.compute()
    if per_file:
        result["files"] = sorted(rows, key=lambda r: r["index"])
    return result


def main(argv=None):
    """python -m audiotokenization_amd.evaluate: extract.py's dataset arguments, --batch (default 16), --per_file,
    --stoi [--stoi_clean ref|rec] and --json OUT (the result dict; printed when absent)."""
    import argparse

    p = argparse.ArgumentParser(description="BigCodec round-trip quality metrics on MI355X (inference_full.py)")
    p.add_argument("--dataset_root", type=str, default="../../datasets")
    p.add_argument("--save_path", type=str, required=True, help="run directory with hydra/config.yaml and last.ckpt")
    p.add_argument("--duration", type=float, default=None)
    p.add_argument("--sample_rate", type=int, default=16000)
    p.add_argument("--dataset_path", type=str, default="LibriTTS")
    p.add_argument("--ext_audio", type=str, default=".flac")
    p.add_argument("--subsets", type=str, nargs="+", required=True)
    p.add_argument("--batch", type=int, default=16, help="clips per ragged round trip")
    p.add_argument("--per_file", action="store_true", help="one row per file under \"files\"")
    p.add_argument("--stoi", action="store_true", help="also STOI (\"stoi\", \"stoi_short_clips\")")
    p.add_argument("--stoi_clean", type=str, default="ref", choices=("ref", "rec"),
                   help="STOI's clean signal: the input (ref, the standard order) or the reconstruction (rec, "
                        "inference_full.py:724)")
    p.add_argument("--json", type=str, default=None, help="write the result here")
    a = p.parse_args(argv)
    if a.batch < 1:
        print(f"Error: --batch must be >= 1 (got {a.batch})")
        return 1
    if not os.path.isdir(a.save_path):
        print(f"Error: Model save path does not exist: {a.save_path}")
        return 1
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    lm = build_lm(a.save_path, device)
    items = find_items(a.dataset_root, a.subsets, a.dataset_path, a.ext_audio)
    if not items:
        print("Error: Dataset is empty. Check dataset root, subset names, and file structure.")
        return 1
    paths = [item_path(subset_path, fileid, a.ext_audio) for _, subset_path, fileid in items]
    result = evaluate_round_trip(lm, paths, batch=a.batch, sample_rate=a.sample_rate, duration=a.duration,
                                 device=device, per_file=a.per_file, stoi=a.stoi, stoi_clean=a.stoi_clean)
    text = json.dumps(result, indent=1)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(text + "\n")
    extra = f", stoi {result['stoi']:.4f}" if a.stoi else ""
    print(text if not a.json else f"{result['clips']} clips: si_snr {result['si_snr']:.3f} dB, mel_distance "
          f"{result['mel_distance']:.4f}, norm_perplexity {result['norm_perplexity']:.4f}{extra} -> {a.json}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
