#!/usr/bin/env python3
"""Cost of the round-trip quality metrics on bench config 3's shape.

Workload: --batch clips of --seconds at --rate (64 x 10 s at 24 kHz, bc_synth_clips white noise), the default model
with synthetic weights at the default precision.  Three arms in one process, each warmed once and then timed --reps
times with device events around the whole arm, between two synchronisations:

  round_trip   encoder -> VQ -> decoder of the batch (the step whose output the metrics judge)
  metrics      RoundTripMetrics.update(x, x_rec, codes=...): SI-SNR, the seven log-mel resolutions, the code histogram
  torch        the same quantities composed from torch-ROCm operators: torch.stft + matmul + reductions (float32; the
               spectrograms go through HBM), SI-SNR with float64 accumulation, torch.bincount

  metrics_stoi (--stoi) the metrics arm with STOI on (RoundTripMetrics(stoi=True)): its row adds stoi_ms, the median
               over the metrics arm's, and no torch composition of STOI is written

A last pass of the metrics arm runs under the launch timers and reports each kernel's summed time.  The torch arm's
peak allocation is reported next to the metrics arm's.  One JSON line per arm; --out also writes them to a file.
Reads nothing outside the tree; needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--rate", type=int, default=24000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--stoi", action="store_true", help="add the metrics_stoi arm (DESIGN.md §21)")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)

    import torch

    from audiotokenization_amd import _lib as L
    from audiotokenization_amd import config, synth
    from audiotokenization_amd import metrics as M
    from audiotokenization_amd.codec import BigCodecDecoder, BigCodecEncoder
    from audiotokenization_amd.extract import synth_batch

    if not torch.cuda.is_available():
        print("metrics_throughput: no HIP device (this measurement has no CPU path)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    L.load()
    cfg = config.preset("default")
    enc = BigCodecEncoder(**config.encoder_kwargs(cfg.model.codec_encoder))
    dec = BigCodecDecoder(**config.decoder_kwargs(cfg.model.codec_decoder))
    for m, prefix in ((enc, "encoder."), (dec, "decoder.")):
        syn = synth.synth_state_dict({prefix + k: v for k, v in m.state_dict().items()})
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in syn.items()}, strict=True)
        m.eval().to(dev)
    size = cfg.model.codec_decoder.codebook_size
    n = int(round(a.seconds * a.rate))
    x = synth_batch(a.batch, n, 0, dev)
    state = {}

    def round_trip():
        post, codes, _ = dec(enc(x), vq=True)
        state["rec"], state["codes"] = dec(post, vq=False), codes

    rtm = M.RoundTripMetrics(a.rate, size)

    def metrics():
        rtm.update(x, state["rec"], codes=state["codes"])

    fbs = [(nf, torch.hann_window(nf, periodic=True, device=dev), M.mel_filterbank(a.rate, nf, nm, dev))
           for nf, nm in zip(rtm.window_lengths, rtm.n_mels)]
    tstate = {"counts": torch.zeros(size, dtype=torch.int64, device=dev)}

    def torch_composition():
        r, c = x[:, 0], state["rec"][:, 0]
        t, q = r.double() - r.double().mean(1, keepdim=True), c.double() - c.double().mean(1, keepdim=True)
        alpha = ((q * t).sum(1, keepdim=True) + M.SI_SNR_EPS) / ((t * t).sum(1, keepdim=True) + M.SI_SNR_EPS)
        s = alpha * t
        snr = 10 * torch.log10(((s * s).sum(1) + M.SI_SNR_EPS) / (((s - q) ** 2).sum(1) + M.SI_SNR_EPS))
        mel = 0.0
        for nf, win, fb in fbs:
            lr, lc = (torch.matmul(fb, torch.stft(v, nf, hop_length=nf // 4, window=win, center=True, pad_mode="reflect",
                                                  return_complex=True).abs()).clamp(min=rtm.clamp_eps).log10()
                      for v in (r, c))
            mel = mel + (lr - lc).abs().mean((1, 2))
        flat = state["codes"].reshape(-1)
        tstate["counts"] += torch.bincount(flat[(flat >= 0) & (flat < size)], minlength=size)
        tstate["snr"], tstate["mel"] = snr, mel

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    arms = {"round_trip": round_trip, "metrics": metrics, "torch": torch_composition}
    if a.stoi:
        rtm_stoi = M.RoundTripMetrics(a.rate, size, stoi=True)
        arms["metrics_stoi"] = lambda: rtm_stoi.update(x, state["rec"], codes=state["codes"])
    lines = []
    with torch.no_grad():
        for fn in arms.values():  # warm-up, in order: the metrics arms read the round trip's output
            timed(fn)
        ms, peak = {k: [] for k in arms}, {}
        for _ in range(a.reps):
            for name, fn in arms.items():
                t, mib = timed(fn)
                ms[name].append(t)
                peak[name] = mib
        med = {k: statistics.median(v) for k, v in ms.items()}
        pc = rtm.per_clip()
        agree = {"si_snr_max_abs_diff_db": float((pc["si_snr"].double() - tstate["snr"]).abs().max()),
                 "mel_distance_max_abs_diff": float((pc["mel_distance"].double() - tstate["mel"].double()).abs().max())}
        tm = L.KernelTimer()
        L.set_timer(tm)
        try:
            metrics()
            summ = tm.summary()
        finally:
            L.set_timer(None)
        for name in arms:
            row = {"arm": name, "batch": a.batch, "seconds": a.seconds, "rate": a.rate, "precision": L.precision_name(),
                   "pass_ms": [round(v, 2) for v in ms[name]], "median_ms": round(med[name], 2),
                   "peak_alloc_mib": round(peak[name], 1)}
            if name == "metrics":
                row.update(share_of_round_trip=round(med["metrics"] / med["round_trip"], 4),
                           vs_torch=round(med["torch"] / med["metrics"], 3),
                           kernels_ms={k: round(d["ms_total"], 3) for k, d in sorted(summ.items())}, **agree)
            if name == "metrics_stoi":
                res = rtm_stoi.compute()
                tm = L.KernelTimer()
                L.set_timer(tm)
                try:
                    arms[name]()
                    row["kernels_ms"] = {k: round(d["ms_total"], 3) for k, d in sorted(tm.summary().items())}
                finally:
                    L.set_timer(None)
                row.update(stoi_ms=round(med["metrics_stoi"] - med["metrics"], 2),
                           share_of_round_trip=round(med["metrics_stoi"] / med["round_trip"], 4), stoi=res["stoi"],
                           stoi_short_clips=res["stoi_short_clips"])
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
