"""Time the Conformer-STFT family on the MI355X (bench.py keeps measuring the BigCodec flagship):

    python tools/conformer_bench.py [--batch 64] [--seconds 10] [--steps 7] [--warmup 3] [--out FILE]

With the `conformer` preset and synthetic weights at batch x seconds of 16 kHz audio it reports
  * encode + VQ and the full round trip: median ms per step and audio seconds per second;
  * the launches one ConformerLayer makes, by op;
  * every kernel of csrc/conformer.hip alone at the model's shapes: median ms;
and, beside each number, the same computation as a plain torch-ROCm float32 composition on the GPU (the test-side
restatement tests/conformer_ref.py moved to the device).  The composition is the comparison, not a threshold.
Times are HIP-event medians over --steps runs after --warmup runs of the same shapes."""
from __future__ import annotations

import argparse
import collections
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import conformer_ref as R  # noqa: E402
from audiotokenization_amd import _lib as L  # noqa: E402
from audiotokenization_amd import config as cfgmod  # noqa: E402
from audiotokenization_amd import conformer as cf  # noqa: E402
from audiotokenization_amd import ops, synth  # noqa: E402
from audiotokenization_amd.extract import synth_batch  # noqa: E402
from audiotokenization_amd.lightning_shim import CodecLightningModule  # noqa: E402


def median_ms(fn, steps, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


class CountingOps:
    """The torch.ops.bigcodec namespace with a call counter per op."""

    def __init__(self, ns):
        self.ns, self.counts = ns, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.ns, name)

        def call(*a, **k):
            self.counts[name] += 1
            return fn(*a, **k)
        return call


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("conformer_bench: needs a HIP device (no fallback)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.batch, int(a.seconds * 16000)
    lm = CodecLightningModule(cfgmod.preset("conformer"))
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(lm.state_dict()).items()}
    lm.load_state_dict(sd, strict=True)
    lm.eval().to(dev)
    esd = {k[len("encoder."):]: v.to(dev) for k, v in sd.items() if k.startswith("encoder.")}
    dsd = {k[len("decoder."):]: v.to(dev) for k, v in sd.items() if k.startswith("decoder.")}
    ek = cfgmod.encoder_kwargs(lm.cfg.model.codec_encoder)
    dk = cfgmod.decoder_kwargs(lm.cfg.model.codec_decoder)
    x = synth_batch(B, T, 0, dev)
    audio_s = B * T / 16000.0
    say(f"conformer preset, {B} x {a.seconds:g} s ({T} samples, {T // 200} frames), precision {L.precision_name()}, "
        f"{torch.cuda.get_device_name(0)}; median [min, max] of {a.steps} after {a.warmup} warm-up runs")

    def enc_vq():
        return lm.decoder(lm.encoder(x), vq=True)

    def round_trip():
        post, codes, _ = enc_vq()
        return lm.decoder(post, vq=False)

    def ref_enc_vq():
        return R.quantize(dsd, R.encoder(esd, ek, x))

    def ref_round_trip():
        return R.decoder(dsd, dk, ref_enc_vq()[0])

    for name, ours, theirs in (("encode + VQ", enc_vq, ref_enc_vq), ("round trip", round_trip, ref_round_trip)):
        m, lo, hi = median_ms(ours, a.steps, a.warmup)
        say(f"{name:12s} HIP kernels     {m:9.3f} ms [{lo:.3f}, {hi:.3f}]  {audio_s / m * 1e3:10.1f} audio-s/s")
        try:
            m2, lo2, hi2 = median_ms(theirs, a.steps, a.warmup)
            say(f"{name:12s} torch fp32 ops  {m2:9.3f} ms [{lo2:.3f}, {hi2:.3f}]  {audio_s / m2 * 1e3:10.1f} audio-s/s"
                f"   (ours / torch {m / m2:.2f})")
        except Exception as e:  # the comparison is not the product: report and go on
            say(f"{name:12s} torch fp32 ops  failed: {type(e).__name__}: {e}")

    # launches of one layer
    real = ops.load
    counter = CountingOps(real())
    ops.load = lambda: counter
    try:
        with torch.no_grad():
            h = torch.randn(2, 256, 50, device=dev)
            lm.encoder.conformer_backbone.layers[0](h, lm.encoder.conformer_backbone.freqs_cis)
    finally:
        ops.load = real
    say(f"launches of one ConformerLayer: {sum(counter.counts.values())} ("
        + ", ".join(f"{k} {v}" for k, v in sorted(counter.counts.items())) + ")")

    # every new kernel alone, at the model's shapes
    Fr, dim, H, D, hid, nfft, hop = T // 200, 256, 8, 32, 768, 800, 200
    ns = ops.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    w = torch.hann_window(nfft)
    basis_t = torch.from_numpy(cf.stft_basis_t(w, nfft).astype(np.float32)).to(dev)
    basis_i = torch.from_numpy(cf.istft_basis(w, nfft).astype(np.float32)).to(dev)
    wd = w.to(dev)
    h = rnd(B, dim, Fr)
    gain = (torch.rand(dim, generator=g) + 0.5).to(dev)
    glu_in, dw_w, dw_b = rnd(B, 2 * dim, Fr), rnd(dim, 1, 31), rnd(dim)
    ff = rnd(B, 2 * hid, Fr)
    qkv = rnd(B, 3 * dim, Fr)
    fc = R.freqs_cis(D, 8192, 500.0)
    rope, fcd = torch.view_as_real(fc).contiguous().to(dev), fc[:Fr].to(dev)
    qkv_btc = qkv.transpose(1, 2).contiguous()
    xp = rnd(B, nfft + 2, Fr)
    kernels = [
        ("stft_frames", lambda: ns.stft_frames(x[:, 0], basis_t, nfft, hop, nfft), lambda: R.stft_features(x, wd, nfft, hop)),
        ("rmsnorm", lambda: ns.rmsnorm(h, gain, 1e-6, False),
         lambda: R.rmsnorm(h.transpose(1, 2), 1e-6, gain).transpose(1, 2).contiguous()),
        ("dwconv_glu", lambda: ns.dwconv_glu(glu_in, dw_w, dw_b, 15), lambda: R.depthwise(F.glu(glu_in, dim=1), dw_w, dw_b, False)),
        ("swiglu", lambda: ns.swiglu(ff), lambda: F.silu(ff[:, :hid]) * ff[:, hid:]),
        ("attention", lambda: ns.attention(qkv, rope, H, False), lambda: R.attention_core(qkv_btc, fcd, H, False)),
        ("istft_head", lambda: ns.istft_head(xp, basis_i, wd, hop), lambda: R.istft_head(xp, wd, nfft, hop)),
    ]
    for name, ours, theirs in kernels:
        m, lo, hi = median_ms(ours, a.steps, a.warmup)
        try:
            m2, lo2, hi2 = median_ms(theirs, a.steps, a.warmup)
            say(f"{name:12s} kernel {m:8.3f} ms [{lo:.3f}, {hi:.3f}]   torch fp32 ops {m2:8.3f} ms [{lo2:.3f}, {hi2:.3f}]"
                f"   (ours / torch {m / m2:.2f})")
        except Exception as e:
            say(f"{name:12s} kernel {m:8.3f} ms [{lo:.3f}, {hi:.3f}]   torch fp32 ops failed: {type(e).__name__}: {e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
