"""STOI on the GPU (csrc/stoi.hip, audiotokenization_amd/metrics.py, evaluate.py) against the float64 oracle of
tests/stoi_ref.py on the inputs of tests/test_stoi_host.py, whose header states the input conditions.

The score tolerance is 4 x the float32 numpy pipeline's own error against float64 on the same clips, the largest over
the batch, recomputed here (the rule of test_gpu_metrics.test_logmel_l1_vs_oracle); kept frame counts are exact.

Measured on an MI355X: see DESIGN.md section 21.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stoi_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import metrics as M
from test_stoi_host import EDGE, batch_case, edge_case, make_batch, make_clip

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_stoi(clean, proc, lens, fs, dev):
    """(scores, kept) of torch.ops.bigcodec.stoi as two host tensors; lens None: every clip fills the row."""
    from audiotokenization_amd import ops

    up, down = M.stoi_resample_ratio(fs)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    filt = None if up == down else M.stoi_resample_filter(fs, dev)
    score, kept = ops.load().stoi(clean.to(dev).contiguous(), proc.to(dev).contiguous(), ld, filt, M.stoi_basis(dev), up,
                                  down)
    return score.cpu(), kept.cpu()


def check_against_oracle(case, fs, dev, what):
    score, kept = gpu_stoi(case["clean"], case["proc"], case["lens"], fs, dev)
    err = np.abs(score.double().numpy() - case["want"])
    bound = 4 * case["f32_err"].max()
    print(f"{what}: float64 {case['want']}, GPU {score.tolist()}, GPU |error| {err}, float32 pipeline error "
          f"{case['f32_err']}, bound {bound:.3e}, kept {kept.tolist()}")
    assert kept.tolist() == [inf["kept"] for inf in case["info"]]
    assert (err <= bound).all(), (err, bound)
    return score, kept


@pytest.mark.parametrize("fs", [16000, 10000])
def test_stoi_vs_oracle(dev, fs):
    """One ragged batch: leading silence, a -50 dB stretch and a zero tail (50 of 77 frames kept); one gap (41 of 52);
    no silence at 33 frames (3 segments) and at exactly 31 frames (1 segment); noise at 20 dB and 0 dB.  At 10 kHz the
    resampler is not launched."""
    check_against_oracle(batch_case(fs), fs, dev, f"stoi fs {fs}")


def test_too_short(dev):
    """29 STFT frames (6552 samples at 16 kHz: 30 frames), and 38 frames of which silence removal keeps 30: exactly
    1e-5, as the oracle; a clip of length 0: NaN."""
    case = edge_case(("short", "silenced"))
    assert case["want"].tolist() == [1e-5, 1e-5]
    T = case["clean"].shape[1]
    clean = torch.cat([case["clean"], torch.ones(1, T)])
    proc = torch.cat([case["proc"], torch.ones(1, T)])
    score, kept = gpu_stoi(clean, proc, case["lens"] + [0], 16000, dev)
    assert kept.tolist() == [EDGE["short"][5], EDGE["silenced"][5], 0]
    assert score[:2].view(torch.int32).tolist() == torch.tensor([1e-5, 1e-5]).view(torch.int32).tolist()
    assert torch.isnan(score[2])
    # a clip with no whole frame at all
    score, kept = gpu_stoi(clean[:1, :300], proc[:1, :300], None, 16000, dev)
    assert kept.tolist() == [0] and score.tolist() == [float(np.float32(1e-5))]


def test_tile_edges(dev):
    """32 and 33 STFT frames (the clip's last workgroup owns 16 frames, then 1), a clip whose loudest frame is its
    last, and one whose first two frames are dropped."""
    check_against_oracle(edge_case(("k33", "k34", "loud_last", "drop2")), 16000, dev, "tile edges")


@pytest.mark.parametrize("fs", [16000, 10000])
def test_tails_are_not_read(dev, fs):
    """NaN beyond each clip's own length in both signals changes no bit of the scores or of kept."""
    case = batch_case(fs)
    score, kept = gpu_stoi(case["clean"], case["proc"], case["lens"], fs, dev)
    c2, p2 = case["clean"].clone(), case["proc"].clone()
    for b, n in enumerate(case["lens"]):
        c2[b, n:] = float("nan")
        p2[b, n:] = float("nan")
    score2, kept2 = gpu_stoi(c2, p2, case["lens"], fs, dev)
    assert torch.isfinite(score).all()
    assert torch.equal(score.view(torch.int32), score2.view(torch.int32)) and torch.equal(kept, kept2)


@pytest.mark.parametrize("fs", [16000, 10000])
def test_a_clip_in_a_batch_equals_the_clip_alone(dev, fs):
    case = batch_case(fs)
    score, kept = gpu_stoi(case["clean"], case["proc"], case["lens"], fs, dev)
    for b, n in enumerate(case["lens"]):
        s1, k1 = gpu_stoi(case["clean"][b:b + 1, :n], case["proc"][b:b + 1, :n], None, fs, dev)
        assert s1.view(torch.int32)[0] == score.view(torch.int32)[b] and k1[0] == kept[b], (b, s1, score[b])
    # the Python entry point, (B, 1, T) input
    got = M.stoi(case["clean"].unsqueeze(1).to(dev), case["proc"].unsqueeze(1).to(dev), fs, lengths=case["lens"]).cpu()
    assert torch.equal(got.view(torch.int32), score.view(torch.int32))


def test_op_refuses_bad_arguments(dev):
    from audiotokenization_amd import ops

    ns = ops.load()
    x = torch.zeros(2, 9000, device=dev)
    filt, basis = M.stoi_resample_filter(16000, dev), M.stoi_basis(dev)
    with pytest.raises(ValueError):
        ns.stoi(x, x[:, :8999].contiguous(), None, filt, basis, 5, 8)
    with pytest.raises(ValueError):
        ns.stoi(x, x, None, None, basis, 5, 8)  # resampling without a filter
    with pytest.raises(ValueError):
        ns.stoi(x, x, None, filt[:580].contiguous(), basis, 5, 8)  # an even tap count
    with pytest.raises(ValueError):
        ns.stoi(x, x, None, filt, basis[:, :255].contiguous(), 5, 8)
    with pytest.raises(ValueError):
        ns.stoi(x, x, None, filt, basis, 100, 441)
    with pytest.raises(ValueError):
        ns.stoi(x, x, torch.zeros(1, dtype=torch.int32, device=dev), filt, basis, 5, 8)


def _debug_lm(dev):
    from audiotokenization_amd.config import preset
    from audiotokenization_amd.lightning_shim import CodecLightningModule
    from helpers import synth_load

    lm = CodecLightningModule(preset("debug"))
    synth_load(lm.encoder, "encoder.")
    synth_load(lm.decoder, "decoder.")
    return lm.eval().to(dev)


def test_round_trip_metrics_with_stoi(dev):
    """RoundTripMetrics(stoi=True) and evaluate_round_trip(..., stoi=True, per_file=True) on three ragged clips through
    the debug model: "stoi" equals the oracle applied to the very waveforms the device produced, stoi_clean="rec"
    equals the oracle with its arguments swapped, the row mean equals the summary, and without stoi there is no key."""
    from audiotokenization_amd.evaluate import evaluate_round_trip
    from audiotokenization_amd.extract import BigCodecModel

    lm = _debug_lm(dev)
    size = lm.cfg.model.codec_decoder.codebook_size
    lens = [12000, 9999, 8000]
    clips = [torch.from_numpy(make_clip(n, 16000, 200 + b).astype(np.float32)) for b, n in enumerate(lens)]
    got = evaluate_round_trip(lm, clips, batch=4, sample_rate=16000, per_file=True, stoi=True)
    swapped = evaluate_round_trip(lm, clips, batch=4, sample_rate=16000, stoi=True, stoi_clean="rec")
    plain = evaluate_round_trip(lm, clips, batch=4, sample_rate=16000, per_file=True)
    assert "stoi" not in plain and "stoi_short_clips" not in plain and all("stoi" not in r for r in plain["files"])
    assert {k: v for k, v in got.items() if k not in ("stoi", "stoi_short_clips", "files")} == \
        {k: v for k, v in plain.items() if k != "files"}
    # the same round trip by hand (plan_batches sorts by length: one group of three, shortest first)
    order = sorted(range(3), key=lambda i: lens[i])
    x = torch.zeros(3, 1, max(lens), device=dev)
    for b, i in enumerate(order):
        x[b, 0, :lens[i]] = clips[i].to(dev)
    slens = [lens[i] for i in order]
    with torch.no_grad():
        out = BigCodecModel(lm, reconstruct=True)(x, lengths=slens)
    own = [min(a, b) for a, b in zip(slens, lm.decoder.sample_lengths([int(f) for f in out["frames"]]))]
    xr, xc = x[:, 0].cpu().numpy(), out["x_rec"][:, 0].cpu().numpy()
    fwd = make_batch([(xr[b, :n], xc[b, :n]) for b, n in enumerate(own)], 16000)
    rev = make_batch([(xc[b, :n], xr[b, :n]) for b, n in enumerate(own)], 16000)
    for name, case, res in (("ref", fwd, got), ("rec", rev, swapped)):
        bound = 4 * case["f32_err"].max()
        print(f"round trip stoi_clean={name}: GPU {res['stoi']}, oracle {case['want']} mean {case['want'].mean()}, float32 "
              f"pipeline error {case['f32_err']}, bound {bound:.3e}, margins "
              f"{[inf['margin_db'] for inf in case['info']]}")
        assert min(inf["margin_db"] for inf in case["info"]) >= 0.05
        assert abs(res["stoi"] - case["want"].mean()) <= bound
        assert res["stoi_short_clips"] == 0 and res["clips"] == 3
    rows = got["files"]
    assert [r["index"] for r in rows] == [0, 1, 2]
    bound = 4 * fwd["f32_err"].max()
    for i, r in enumerate(rows):
        assert abs(r["stoi"] - fwd["want"][order.index(i)]) <= bound
    assert abs(np.mean([r["stoi"] for r in rows]) - got["stoi"]) < 1e-6
    # the class itself: per_clip() and the short-clip count
    m = M.RoundTripMetrics(16000, size, stoi=True)
    short = edge_case(("short", "k33"))
    m.update(short["clean"].to(dev), short["proc"].to(dev), lengths=short["lens"])
    res = m.compute()
    assert res["stoi_short_clips"] == 1 and m.per_clip()["stoi"].shape == (2,)
    assert abs(res["stoi"] - (1e-5 + short["want"][1]) / 2) <= 4 * short["f32_err"].max()


CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from audiotokenization_amd import _lib as L
from test_gpu_stoi import gpu_stoi
from test_stoi_host import CASES, build_pair
import numpy as np
lib = L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
out = {{}}
for fs in (16000, 10000):
    spec = CASES[fs]
    clean = np.zeros((len(spec["clips"]), spec["T"]), np.float32)
    proc = np.zeros_like(clean)
    lens = []
    for b, (shape, n, snr, _, _) in enumerate(spec["clips"]):
        clean[b, :n], proc[b, :n] = build_pair(shape, n, fs, snr)
        lens.append(n)
    score, kept = gpu_stoi(torch.from_numpy(clean), torch.from_numpy(proc), lens, fs, dev)
    out[str(fs)] = {{"status": L.debug_status(), "bits": score.view(torch.int32).tolist(), "kept": kept.tolist()}}
print("DEBUG_RESULT " + json.dumps(out))
"""


def test_stoi_in_the_bounds_checked_build(dev):
    """The batches of test_stoi_vs_oracle on the debug library (a child process with BIGCODEC_DEBUG=1): no computed
    index fails its check, and the scores are bit-identical to the product library's."""
    from audiotokenization_amd import build_lib

    dlib = os.path.join(build_lib.DEBUG_DIR, "libbigcodec_hip.so")
    assert os.path.exists(dlib), "debug library not built (python audiotokenization_amd/build_lib.py --debug)"
    assert build_lib.lib_digest(dlib) == build_lib._digest(build_lib._paths(True)[2]), "debug library older than the sources"
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BIGCODEC_DEBUG="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1]
    res = json.loads(line[len("DEBUG_RESULT "):])
    print(res)
    for fs in (16000, 10000):
        case = batch_case(fs)
        score, kept = gpu_stoi(case["clean"], case["proc"], case["lens"], fs, dev)
        assert res[str(fs)]["status"] == [0, 0], res
        assert res[str(fs)]["bits"] == score.view(torch.int32).tolist() and res[str(fs)]["kept"] == kept.tolist()
    assert L.debug_status() is None  # this process runs the product library
