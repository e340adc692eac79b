"""Generate tests/golden/conformer_*.npz from the REFERENCE Conformer-STFT modules (development container only: the
reference never travels):
    python tools/make_golden_conformer.py
Data only: synthetic clips (synth.synth_clips), the reference's outputs and layer-0 intermediates on them, the fp64
top-2 VQ gap per frame, the RoPE table and the reference's state_dict key names and shapes.  Weights are not stored:
both sides synthesise them from the counter-hash spec (synth.synth_state_dict).

The clip offset of each fixture is the first one whose smallest top-2 gap is at least 10 x helpers.GAP_TOL, so the
near-tie allowance of helpers.index_mismatches is empty on these fixtures: any flipped index fails."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import refimport  # noqa: E402
from audiotokenization_amd import config as cfgmod  # noqa: E402
from audiotokenization_amd import synth  # noqa: E402
from helpers import GAP_TOL, top2_gap  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
MAX_FILE = 1.5e6


def build_ref(ref, name, **ov):
    cfg = cfgmod.preset(name, **ov)
    ek = cfgmod.encoder_kwargs(cfg.model.codec_encoder)
    dk = cfgmod.decoder_kwargs(cfg.model.codec_decoder)
    enc = ref.encoder.ConformerEncoderSTFT(**ek)
    dec = ref.decoder.ConformerDecoderISTFT(**dk)
    for m, prefix in ((enc, "encoder."), (dec, "decoder.")):
        full = {prefix + k: v for k, v in m.state_dict().items()}
        syn = synth.synth_state_dict(full, seed=0)
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in syn.items()}, strict=True)
        m.eval()
    return enc, dec, ek, dk


def ct(t):
    """(B, T, C) -> (B, C, T) array."""
    return t.detach().transpose(1, 2).contiguous().numpy()


def trace_layer0(model, rec, prefix, conv_first):
    """Hooks that record layer 0's four sub-block outputs (the input of the next norm / the layer's output) and the
    attention output before out_proj."""
    l0 = model.conformer_backbone.layers[0]
    second = "attn_norm_in" if conv_first else "conv_norm_in"
    names = {"ffn1_norm_in": "conv" if conv_first else "attn_out", second: "ffn1",
             "ffn2_norm_in": "attn_out" if conv_first else "conv"}
    hs = []
    for mod, key in names.items():
        hs.append(getattr(l0, mod).register_forward_pre_hook(
            lambda m, a, key=key: rec.__setitem__(prefix + key, ct(a[0]))))
    hs.append(l0.self_attn.out_proj.register_forward_pre_hook(lambda m, a: rec.__setitem__(prefix + "attn", ct(a[0]))))
    hs.append(l0.register_forward_hook(lambda m, a, o: rec.__setitem__(prefix + "ffn2", o.detach().numpy())))
    return hs


@torch.no_grad()
def case(ref, name, tag, n_clips, n_samples, intermediates, **ov):
    enc, dec, ek, dk = build_ref(ref, name, **ov)
    fvq = dec.quantizer.layers[0]
    for clip0 in range(64):
        x = torch.from_numpy(synth.synth_clips(n_clips, n_samples, clip0=clip0)).unsqueeze(1)
        gap = top2_gap(fvq.in_proj(enc(x).transpose(1, 2)).transpose(1, 2), fvq.codebook.weight)
        if float(gap.min()) >= 10 * GAP_TOL:
            break
    assert float(gap.min()) >= 10 * GAP_TOL, f"{tag}: no clip offset below 64 clears the gap condition"
    rec = {}
    hs = trace_layer0(enc, rec, "enc_", True) + trace_layer0(dec, rec, "dec_", False)
    hs.append(enc.input_proj.register_forward_pre_hook(lambda m, a: rec.__setitem__("enc_stft", a[0].detach().numpy())))
    hs.append(enc.input_norm.register_forward_hook(lambda m, a, o: rec.__setitem__("enc_input_norm", ct(o))))
    hs.append(dec.head.register_forward_hook(lambda m, a, o: rec.__setitem__("dec_x_pred", o[1].detach().numpy())))
    latent = enc(x)
    post, codes, _ = dec(latent, vq=True)
    wav = dec(post, vq=False)
    for h in hs:
        h.remove()
    out = dict(latent=latent.numpy(), codes=codes.numpy(), post=post.numpy(), wav=wav.numpy(), gap=gap,
               rope=torch.view_as_real(enc.conformer_backbone.freqs_cis[: latent.shape[2]]).numpy())
    if intermediates:
        out.update(rec)
    keys = {side: [[k, list(v.shape)] for k, v in m.state_dict().items()] for side, m in (("encoder", enc), ("decoder", dec))}
    meta = dict(model=name, overrides=ov, n_clips=n_clips, n_samples=n_samples, clip0=clip0, torch=torch.__version__,
                min_gap=float(gap.min()), encoder_kwargs=ek, decoder_kwargs=dk, state_dict=keys)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    size = os.path.getsize(path)
    assert size <= MAX_FILE, f"{path}: {size} bytes"
    print(f"{tag}: clip0 {clip0}, min gap {gap.min():.2e}, {size} bytes")
    return size


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = refimport.load()
    total = case(ref, "conformer_debug", "conformer_debug", 2, 6400, True)
    total += case(ref, "conformer_debug", "conformer_debug_causal", 2, 6400, True, causal=True)
    total += case(ref, "conformer", "conformer_base", 2, 16000, False)
    assert total < 4e6, total


if __name__ == "__main__":
    main()
