#!/usr/bin/env python3
"""Ragged-batch encode throughput on a corpus-like length mix (DESIGN.md "Ragged batches").

Workload: --clips synthetic clips (bc_synth_clips white noise) with lengths drawn uniformly from [--min-s, --max-s]
seconds at 24 kHz by numpy's default_rng(--seed); the default model with synthetic weights, the default precision
(x6).  Arms, all in one process, after one untimed pass of every arm (so every shape has run once), alternating:

  per_clip   every clip alone, encoder + VQ at B = 1: what extract.run_extraction(batch=1) does per file
  ragged_N   extract.plan_batches(lengths, N) groups, each assembled into a zero-padded batch and encoded with
             lengths (the assembly is inside the timed pass, as it is in run_extraction(batch=N))

Each pass is timed with device events around the whole pass, between two synchronisations.  audio-s/s counts REAL
samples only; `padded` is the share of a ragged arm's batch columns that is padding.  A last untimed-for-rate pass per
ragged arm runs under the launch timers (bc_launch_timer_*) and reports bc_zero_tail's launches and summed kernel time
against the pass time measured with the timers off.  One JSON line per arm; --out also writes them to a file.
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
    p.add_argument("--clips", type=int, default=256)
    p.add_argument("--min-s", type=float, default=2.0)
    p.add_argument("--max-s", type=float, default=20.0)
    p.add_argument("--rate", type=int, default=24000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)

    import numpy as np
    import torch

    from audiotokenization_amd import _lib as L
    from audiotokenization_amd import config, synth
    from audiotokenization_amd.codec import BigCodecDecoder, BigCodecEncoder
    from audiotokenization_amd.extract import plan_batches, synth_batch

    if not torch.cuda.is_available():
        print("ragged_throughput: no HIP device (this measurement has no CPU path)", file=sys.stderr)
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

    rng = np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_s * a.rate), int(a.max_s * a.rate), size=a.clips, endpoint=True).tolist()
    clips = [synth_batch(1, n, b, dev) for b, n in enumerate(lengths)]  # (1, 1, n) each, on the device
    real_s = sum(lengths) / a.rate

    def per_clip():
        frames = 0
        for x in clips:
            codes = dec(enc(x), vq=True)[1]
            frames += codes.shape[-1]
        return frames

    def ragged(batch):
        groups = plan_batches(lengths, batch)

        def run():
            frames = 0
            for g in groups:
                lens = [lengths[i] for i in g]
                x = torch.zeros((len(g), 1, max(lens)), device=dev)
                for j, i in enumerate(g):
                    x[j, :, :lens[j]] = clips[i][0]
                codes = dec(enc(x, lengths=lens), vq=True)[1]
                frames += sum(enc.frame_lengths(lens))
            return frames
        cols = sum(len(g) * max(lengths[i] for i in g) for g in groups)
        return run, 1.0 - sum(lengths) / cols, len(groups)

    arms = {"per_clip": (per_clip, 0.0, a.clips)}
    for b in a.batches:
        arms[f"ragged_{b}"] = ragged(b)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frames = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), frames

    lines = []
    with torch.no_grad():
        frames_of = {}
        for name, (fn, _, _) in arms.items():  # warm-up: every shape of every arm once
            frames_of[name] = timed(fn)[1]
        ms = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, (fn, _, _) in arms.items():
                ms[name].append(timed(fn)[0])
        base = statistics.median(ms["per_clip"])
        for name, (fn, padded, forwards) in arms.items():
            med = statistics.median(ms[name])
            row = {"arm": name, "clips": a.clips, "forwards": forwards, "real_audio_s": round(real_s, 1),
                   "frames": frames_of[name], "pass_ms": [round(v, 1) for v in ms[name]], "median_ms": round(med, 1),
                   "audio_s_per_s": round(real_s / (med / 1e3), 1), "padded": round(padded, 4),
                   "vs_per_clip": round(base / med, 3), "precision": L.precision_name(),
                   "lengths_s": [a.min_s, a.max_s], "seed": a.seed}
            if name != "per_clip":  # a pass of its own under the launch timers (they slow the host: not a rate)
                tm = L.KernelTimer()
                L.set_timer(tm)
                try:
                    fn()
                    summ = tm.summary()
                finally:
                    L.set_timer(None)
                zt = summ.get("zero_tail_kernel", dict(launches=0, ms_total=0.0))
                row.update(zero_tail_launches=zt["launches"], zero_tail_ms=round(zt["ms_total"], 2),
                           zero_tail_share_of_pass=round(zt["ms_total"] / med, 4),
                           kernel_ms_under_timer=round(sum(d["ms_total"] for d in summ.values()), 1))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
