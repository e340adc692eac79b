"""Ragged batches on the GPU: bc_zero_tail against torch, then the encoder and decoder with `lengths` against the CPU
oracle run on every clip ALONE (the reference's own job: one file per forward), the independence properties, token
decoding and the extraction CLI with --batch."""
import os

import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import extract, ops, tokens
from helpers import assert_close_rel, build_models, index_mismatches, top2_gap, torch_sd
from oracle import bigcodec_oracle as O
from test_ragged_host import CASES, IDS, ragged_clips, ragged_lengths

pytestmark = pytest.mark.gpu


# ---- the kernel ---------------------------------------------------------------------------------------------------
def _length_sets(B, T):
    """Length vectors for (B, ., T): 0, T, T - 1 and T - 2 in turn; tails starting at every residue mod 4 (four
    consecutive starts per clip position); values outside [0, T], which the kernel clamps."""
    sets = [[(0, T, T - 1, max(T - 2, 0))[(b + r) % 4] for b in range(B)] for r in range(4)]
    sets += [[min(T, max(0, T // 2 + k + b)) for b in range(B)] for k in range(4)]
    sets += [[(T + 3, -2, T // 3, T)[b % 4] for b in range(B)]]
    return sets


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "view+4B"])
@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 48, 130), (2, 96, 513), (4, 16, 1001)])
def test_zero_tail_kernel(dev, shape, dual, unaligned):
    """zero_tail_ == `y[b, :, clamp(lens[b], 0, T):] = 0` in torch: the prefix bit for bit, the tail exactly +0.0
    although it held NaN and Inf; y2 alike; an unaligned (contiguous, 4 bytes off) tensor takes the scalar stores."""
    B, C, T = shape
    ns = ops.load()
    g = torch.Generator().manual_seed(B * 1000 + T)

    def fresh():
        n = B * C * T
        if unaligned:
            return torch.empty(n + 1, device=dev)[1:].view(B, C, T)
        return torch.empty(B, C, T, device=dev)

    for lens in _length_sets(B, T):
        clamped = [min(max(v, 0), T) for v in lens]
        host = [torch.randn(B, C, T, generator=g) for _ in range(2)]
        for h in host:
            for b, n in enumerate(clamped):
                h[b, :, n:][..., 0::2] = float("nan")
                h[b, :, n:][..., 1::2] = float("inf")
        ys = []
        for h in host[: 2 if dual else 1]:
            y = fresh()
            y.copy_(h)
            ys.append(y)
        assert (ys[0].data_ptr() % 16 != 0) == unaligned
        want = [h.clone() for h in host]
        for w in want:
            for b, n in enumerate(clamped):
                w[b, :, n:] = 0.0
        lens_d = torch.tensor(lens, dtype=torch.int32).to(dev)
        ns.zero_tail_(ys[0], ys[1] if dual else None, lens_d, T - min(clamped))
        for y, w in zip(ys, want):
            assert torch.equal(y.cpu().view(torch.int32), w.view(torch.int32)), (shape, lens)


def test_zero_tail_refuses_bad_arguments(dev):
    ns = ops.load()
    y = torch.zeros(2, 3, 8, device=dev)
    lens = torch.tensor([4, 8], dtype=torch.int32, device=dev)
    with pytest.raises((ValueError, RuntimeError)):
        ns.zero_tail_(y, None, lens[:1], 4)
    with pytest.raises((ValueError, RuntimeError)):
        ns.zero_tail_(y, None, lens.long(), 4)
    with pytest.raises((ValueError, RuntimeError)):
        ns.zero_tail_(y, torch.zeros(2, 3, 7, device=dev), lens, 4)
    with pytest.raises((ValueError, RuntimeError)):
        ns.zero_tail_(y, None, lens.cpu(), 4)


DEBUG_CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r})
from audiotokenization_amd import _lib as L
from audiotokenization_amd import ops
L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
ok = True
for (B, C, T), lens in [((3, 5, 7), [0, 7, 3]), ((2, 96, 513), [511, 130]), ((4, 16, 1001), [1001, 1, 998, 500])]:
    g = torch.Generator().manual_seed(T)
    h, h2 = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    y, y2 = h.to(dev), h2.to(dev)
    ops.load().zero_tail_(y, y2, torch.tensor(lens, dtype=torch.int32).to(dev), T - min(lens))
    for b, n in enumerate(lens):
        h[b, :, n:] = 0.0
        h2[b, :, n:] = 0.0
    ok = ok and torch.equal(y.cpu(), h) and torch.equal(y2.cpu(), h2)
print("DEBUG_RESULT " + json.dumps({{"status": L.debug_status(), "equal": bool(ok)}}))
"""


def test_zero_tail_in_the_bounds_checked_build():
    """The debug library (BIGCODEC_DEBUG=1, loaded by a child process) carries zero_tail with its index guards: the
    same zeros, and no failed check."""
    import json
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD.format(repo=repo)], env=dict(os.environ, BIGCODEC_DEBUG="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1][len("DEBUG_RESULT "):])
    assert res == {"status": [0, 0], "equal": True}, res


# ---- the models against the per-clip oracle -------------------------------------------------------------------------
_GPU, _REF = {}, {}


def gpu_models(dev, name, ov):
    key = (name, tuple(sorted(ov.items())))
    if key not in _GPU:
        _GPU[key] = build_models(name, device=dev, **ov)
    return _GPU[key]


def reference(dev, name, ov, lengths, clip0=11):
    """Every clip ALONE through the CPU oracle, once per case (shared, never modified): latents, codes, top-2 gaps, the
    post-VQ latents and their waveforms."""
    key = (name, tuple(sorted(ov.items())), tuple(lengths), clip0)
    if key not in _REF:
        enc, dec, esd, dsd, ek, dk = gpu_models(dev, name, ov)
        esd, dsd = torch_sd(esd), torch_sd(dsd)
        x = ragged_clips(lengths, clip0)
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        ref = dict(x=x, lat=[], codes=[], gap=[], post=[], wav=[])
        with torch.no_grad():
            for b, n in enumerate(lengths):
                lat = O.encoder_forward(x[b:b + 1, :, :n], esd, ek)
                post, codes, _, ze = O.fvq_forward(lat, dsd, "quantizer.layers.0.", return_ze=True)
                ref["lat"].append(lat[0])
                ref["codes"].append(codes[0].numpy())
                ref["gap"].append(top2_gap(ze, dsd["quantizer.layers.0._codebook.weight"])[0])
                ref["post"].append(post[0])
        _REF[key] = ref
    return _REF[key]


def reference_wavs(dev, name, ov, lengths):
    ref = reference(dev, name, ov, lengths)
    if not ref["wav"]:
        _, _, _, dsd, _, dk = gpu_models(dev, name, ov)
        with torch.no_grad():
            ref["wav"] = [O.decoder_forward(p[None], torch_sd(dsd), dk)[0] for p in ref["post"]]
    return ref


def check_encoder(dev, name, ov, lengths, clip0=11, what=""):
    enc, dec, *_ = gpu_models(dev, name, ov)
    ref = reference(dev, name, ov, lengths, clip0)
    frames = enc.frame_lengths(lengths)
    with torch.no_grad():
        lat = enc(ref["x"].to(dev), lengths=lengths)
        codes = dec(lat, vq=True)[1]
        torch.cuda.synchronize()
    assert lat.shape[0] == len(lengths) and lat.shape[2] == max(frames) and codes.shape == (1, len(lengths), max(frames))
    lat, codes = lat.cpu(), codes.cpu().numpy()
    worst = 0.0
    for b, f in enumerate(frames):
        assert ref["lat"][b].shape[-1] == f
        assert_close_rel(lat[b, :, :f], ref["lat"][b], 1e-4, f"{what} clip {b} ({lengths[b]} samples) latent", profile=True)
        n_bad, w = index_mismatches(codes[0, b, :f], ref["codes"][b], ref["gap"][b])
        worst = max(worst, w)
    print(f"ragged encoder {what}: {len(lengths)} clips, frames {frames}, worst certified gap {worst:.2e}")


@pytest.mark.parametrize("name,ov", CASES, ids=IDS)
def test_ragged_encoder_equals_the_per_clip_oracle(dev, prec, name, ov):
    """enc(x, lengths)[b, :, :F_b] is the oracle's encode of clip b ALONE, within the project's 1e-4, and so are the
    codes (a differing index only at a certified near-tie; the smallest top-2 gap of these clips is 5.6e-4, far
    above GAP_TOL, so any differing index fails)."""
    enc, *_ = gpu_models(dev, name, ov)
    check_encoder(dev, name, ov, ragged_lengths(int(enc.hop_length)), what=f"{IDS[CASES.index((name, ov))]} [{prec}]")


TILE_LENGTHS = [24000, 23041, 22529]


def test_ragged_encoder_at_tile_boundaries(dev):
    """x6, three clips of about 1 s whose per-layer lengths (enc.frame_lengths(per_layer=True)) end on, or one column
    past, multiples of the kernels' 128- and 256-column tiles while the longest clip runs on, so whole tiles lie past a
    clip's end and others straddle it:
      input and first conv (width 24000): 23041 = 256 * 90 + 1 (and 1 mod 4), 22529 = 256 * 88 + 1
      block 1, C = 96 (12000): 11520 = 256 * 45, 11264 = 256 * 44     block 2, C = 192 (6000): 5760 = 128 * 45, 5632 = 256 * 22
      block 3, C = 384 (3000): 2880, 2816 = 256 * 11                   block 4 / 5 and the ResLSTM: 576 / 563, 115 / 112
    The smallest oracle top-2 gap of these clips (clip0 = 11) is 1.2e-4, measured on the CPU."""
    enc, *_ = gpu_models(dev, "default", {})
    table = enc.frame_lengths(TILE_LENGTHS, per_layer=True)
    assert TILE_LENGTHS[1] % 4 == 1 and [24000, 23041, 22529] in table and [12000, 11520, 11264] in table
    assert [6000, 5760, 5632] in table and [3000, 2880, 2816] in table and table[-1] == [120, 115, 112]
    old = L.precision_mode()
    L.set_precision("x6")
    try:
        check_encoder(dev, "default", {}, TILE_LENGTHS, what="tile boundaries [x6]")
    finally:
        L._mode = old


def test_ragged_independence(dev):
    """What lies past a clip's length does not exist: garbage (NaN, Inf) there gives the bits zeros give, and the
    caller's tensor is not written; lengths = [T] * B gives the bits of lengths=None; and lengths=None launches no
    zero_tail kernel, while a ragged forward launches one per masked producer (a dual output shares it)."""
    enc, dec, *_ = gpu_models(dev, "default", {})
    lengths = ragged_lengths(int(enc.hop_length))
    x = ragged_clips(lengths).to(dev)
    for b, n in enumerate(lengths):
        x[b, :, n:] = 0.0
    junk = x.clone()
    g = torch.Generator().manual_seed(5)
    for b, n in enumerate(lengths):
        t = torch.randn(1, max(lengths) - n, generator=g) * 100.0
        t[:, 0::3] = float("nan")
        t[:, 1::7] = float("inf")
        junk[b, :, n:] = t.to(dev)
    keep = junk.clone()
    with torch.no_grad():
        a = enc(x, lengths=lengths)
        b_ = enc(junk, lengths=lengths)
        full = [max(lengths)] * len(lengths)
        c = enc(x, lengths=full)
        tm = L.KernelTimer()
        L.set_timer(tm)
        try:
            d = enc(x)
            none_summary = tm.summary()
            tm2 = L.KernelTimer()
            L.set_timer(tm2)
            enc(x, lengths=lengths)
            ragged_summary = tm2.summary()
            tm3 = L.KernelTimer()
            L.set_timer(tm3)
            enc(x, lengths=full)
            full_summary = tm3.summary()
        finally:
            L.set_timer(None)
        torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    assert torch.equal(junk.view(torch.int32), keep.view(torch.int32))
    assert torch.equal(c, d)
    assert not any("zero_tail" in k for k in none_summary), sorted(none_summary)
    assert not any("zero_tail" in k for k in full_summary), sorted(full_summary)  # nothing is shorter: no launch either
    n_masked = len(enc.frame_lengths(lengths, per_layer=True)) - 1  # every row but the latent's
    assert ragged_summary["zero_tail_kernel"]["launches"] == n_masked, ragged_summary["zero_tail_kernel"]
    # the decoder alike
    frames = enc.frame_lengths(lengths)
    z = torch.randn(len(frames), 1024, max(frames), generator=g).to(dev) * 0.1
    zj = z.clone()
    for b, f in enumerate(frames):
        z[b, :, f:] = 0.0
        zj[b, :, f:] = float("nan")
    with torch.no_grad():
        w0 = dec.decode(z, lengths=frames)
        w1 = dec(zj, vq=False, lengths=frames)
        w2 = dec.decode(z, lengths=[max(frames)] * len(frames))
        w3 = dec.decode(z)
    assert torch.equal(w0.view(torch.int32), w1.view(torch.int32)) and torch.isnan(zj).any()
    assert torch.equal(w2, w3)


@pytest.mark.parametrize("name,ov", CASES, ids=IDS)
def test_ragged_decoder_equals_the_per_clip_oracle(dev, prec, name, ov):
    """decode(x, lengths=frames) of the oracle's per-clip post-VQ latents, stacked with junk in the tails: each clip's
    [: F_b * hop] meets the project's waveform tolerance (MSE <= 1e-12, max <= 1e-5) against the oracle's decode of
    that clip alone, and the rest of its row is exactly zero."""
    enc, dec, *_ = gpu_models(dev, name, ov)
    lengths = ragged_lengths(int(enc.hop_length))
    ref = reference_wavs(dev, name, ov, lengths)
    frames = enc.frame_lengths(lengths)
    samples = dec.sample_lengths(frames)
    z = torch.randn(len(frames), ref["post"][0].shape[0], max(frames), generator=torch.Generator().manual_seed(2)) * 3.0
    for b, f in enumerate(frames):
        z[b, :, :f] = ref["post"][b]
    with torch.no_grad():
        wav = dec.decode(z.to(dev), lengths=frames).cpu()
    assert wav.shape == (len(frames), 1, max(samples))
    for b, n in enumerate(samples):
        want = ref["wav"][b]
        assert want.shape[-1] == n == frames[b] * int(dec.hop_length)
        err = (wav[b, :, :n] - want).double()
        mse, mx = float((err ** 2).mean()), float(err.abs().max())
        print(f"ragged decoder {name} {ov} [{prec}] clip {b}: mse {mse:.2e} max {mx:.2e}")
        assert mse <= 1e-12 and mx <= 1e-5, (b, mse, mx)
        assert not wav[b, :, n:].any() and not torch.signbit(wav[b, :, n:]).any()


def test_decode_index_files_ragged(dev, tmp_path):
    """decode_index_files(ragged=True) (mixed lengths in one batch) against the default path (equal lengths only,
    here every file alone): the project's waveform tolerance."""
    enc, dec, *_ = gpu_models(dev, "default", {})
    lengths = ragged_lengths(int(enc.hop_length))
    ref = reference(dev, "default", {}, lengths)
    paths = [extract.save_indices(str(tmp_path), "test-clean", f"{i}-1-{i:04d}", c[:, None].astype(np.int16))
             for i, c in enumerate(ref["codes"])]
    plain = tokens.decode_index_files(dec, paths, dev, batch=4)
    ragged = tokens.decode_index_files(dec, paths, dev, batch=4, ragged=True)
    hop = int(dec.hop_length)
    for c, p, r in zip(ref["codes"], plain, ragged):
        assert p.shape == r.shape == (c.shape[0] * hop,)
        err = (r.astype(np.float64) - p.astype(np.float64))
        assert float((err ** 2).mean()) <= 1e-12 and float(np.abs(err).max()) <= 1e-5
    codes, lens = tokens.codes_to_device([tokens.load_indices(p) for p in paths], dev, 8192)
    for w, r in zip(tokens.decode_codes(dec, codes, lens, ragged=True), ragged):
        assert w.shape == (1, r.shape[0])


# ---- the extraction CLI ---------------------------------------------------------------------------------------------
def test_cli_batch_equals_per_file(tmp_path, dev, capsys):
    """--batch 4 on test_extract_cli's FLAC tree: the files, dtypes, shapes and printed counts of --batch 1, and the same
    codes (a differing frame only at a certified near-tie of the per-file latent's oracle VQ)."""
    from audiotokenization_amd.ingest import load_item
    from test_extract_cli import _save_path, _tree

    ids = _tree(str(tmp_path))
    sp, enc, dec = _save_path(str(tmp_path))
    outs = {}
    for batch, folder in ((1, "per_file"), (4, "ragged")):
        rc = extract.main(["--dataset_root", str(tmp_path), "--save_path", sp, "--subsets", "test-clean", "--sample_rate",
                           "24000", "--workers", "2", "--output_folder", folder, "--batch", str(batch)])
        outs[batch] = capsys.readouterr().out
        assert rc == 0
    for out in outs.values():
        assert f"Successfully saved {len(ids)} index files." in out and "Encountered 2 errors." in out

    def listing(folder):
        root = os.path.join(sp, folder)
        return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)

    assert listing("per_file") == listing("ragged") and len(listing("ragged")) == len(ids)
    dsd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    enc.to(dev)
    for rel in listing("ragged"):
        a, b = np.load(os.path.join(sp, "per_file", rel)), np.load(os.path.join(sp, "ragged", rel))
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape and a.ndim == 2
        fid = os.path.basename(rel)[:-4]
        parts = fid.split("_") if "_" in fid else fid.split("-")
        src = os.path.join(str(tmp_path), "LibriTTS", "test-clean", parts[0], parts[1], fid + ".flac")
        wav, _ = load_item(src, 24000, None, None, dev)
        with torch.no_grad():
            lat = enc(wav.unsqueeze(0)).cpu()
            ze = O.fvq_forward(lat, dsd, "quantizer.layers.0.", return_ze=True)[3]
        gap = top2_gap(ze, dsd["quantizer.layers.0._codebook.weight"])[0]
        index_mismatches(b[:, 0], a[:, 0], gap)
