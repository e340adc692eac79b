"""The ResLSTM matrix on the host (no GPU).

1. What the bound tests/test_gpu_lstm_matrix.py applies (lstm_ref.bound: K[prec] times the fp32 CPU error of the case)
   can discriminate: on every matrix case it stays below half the error of an fp32 recurrence on single-plane (bf16)
   operands; against one that only lost the third bf16 plane of W_hh or of h (what a broken x6 split, or an h3 that lost
   its second plane, would compute) the proof is required of the precisions in lstm_ref.LOW_PLANE_PROVEN, which is
   empty, with the figures, in test_bound_discriminates.  The cell loop that computes the degraded recurrences is first
   checked against torch.nn.LSTM in fp64.  test_bidir_bound_discriminates is the same for the bidirectional cases,
   whose faults can sit in five places (either direction's W_hh or h, the reverse-half columns of W_ih).
2. The W_hh pack layouts the kernels read: x6 at H = 1024 and 1536 (tests/test_abi.py has 256 and 512), h3 at all four
   widths, and the per-step fast kernel's (lstm_pack_hh2) at H = 128 and 1024, each under the index map written out
   here from the comments in csrc/lstm_seq.hip and csrc/lstm.hip."""
import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L
from lstm_ref import (BIDIR_SHAPES, FRAG_H, K, LOW_PLANE_PROVEN, SEQ_H, SHAPES, bidir_case, bidir_precs, bound, cpu32,
                      main_case, manual_lstm, planes, ref64, rel_h, rel_h_halves, state_case)

CASES = [main_case(H) for H in sorted(SHAPES)] + [state_case(H) for H in SEQ_H]
BIDIR_CASES = [bidir_case(k) for k in BIDIR_SHAPES]


def _precs(case):
    """Precisions the GPU matrix runs a case in: the carried-state cases on the persistent kernel only."""
    if case.state:
        return ("x6", "h3")
    return ("x6", "h3", "bf16", "fp32") if case.H in SEQ_H else ("fp32",)


def test_planes():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(planes(v, 3), v)
    assert torch.equal(planes(v, 1), v.to(torch.bfloat16).float())
    e2 = float(((planes(v, 2) - v).abs() / v.abs()).max())
    assert 2.0 ** -19 < e2 <= 2.0 ** -16, e2  # two planes: 16 significant bits


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"H{c.H}{'-state' if c.state else ''}")
def test_bound_discriminates(case):
    """What the GPU matrix's bound can tell from fp32 arithmetic, per case and precision.  A precision listed in
    LOW_PLANE_PROVEN must have bound < 1/2 min(drop_w, drop_h), the errors of an fp32 recurrence whose W_hh / whose h
    lost its third bf16 plane.  No precision is: measured here at B = 130 (70 with state), min(drop_w, drop_h) /
    max(cpu32) is 4.6 (H = 48), 4.0 (64), 11 (128), 5.3 (256), 4.5 (512), 5.5 (768), 4.1 (1024), 3.3 (1536) and
    8.0 / 6.3 / 3.6 / 3.5 with state, while the kernels -- native fp32 MFMA and libm nonlinearities included -- come
    within 1.6x (2.3x for x6's h_n) of cpu32 on the MI355X, so K = 3.2 / 4.6 would need 6.4 / 9.2.  Every other
    precision must have bound < 1/2 of the error with a single-plane (bf16) W_hh and with a single-plane h, which is
    1.7e-3 .. 1.7e-2 here: a recurrence on bf16 operands fails by three orders of magnitude, a dropped low plane
    (2.8e-6 .. 2.1e-5 against bounds of 1.8e-6 .. 4.7e-6) fails on most cases but is not guaranteed to."""
    ref = ref64(case)
    m64 = manual_lstm(case, torch.float64)
    for a, b in zip(m64, ref):  # the written-out cell loop is torch's LSTM
        assert rel_h(a, b) < 1e-12
    err = {}
    for name, n in (("drop", 2), ("one", 1)):
        err[name + "_w"] = rel_h(manual_lstm(case, torch.float32, fw=lambda v: planes(v, n))[0], ref[0])
        err[name + "_h"] = rel_h(manual_lstm(case, torch.float32, fh=lambda v: planes(v, n))[0], ref[0])
    drop, one = min(err["drop_w"], err["drop_h"]), min(err["one_w"], err["one_h"])
    c32 = cpu32(case)
    print(f"H {case.H} layers {case.layers} T {case.T} B {case.B} whh_scale {case.whh_scale} state {case.state}: max |h| "
          f"{float(ref[0].abs().max()):.3f} cpu32 y {c32[0]:.2e} h_n {c32[1]:.2e} c_n {c32[2]:.2e} " +
          " ".join(f"{k} {v:.2e}" for k, v in err.items()) + f" drop / cpu32 {drop / max(c32):.1f}; bounds " +
          " ".join(f"{p} {bound(case, p):.2e} (drop = {drop / bound(case, p):.2f} x bound)" for p in _precs(case)))
    assert max(c32) < drop < 0.01 * one
    for prec in _precs(case):
        assert K[prec] >= 1.0
        if prec in LOW_PLANE_PROVEN:
            assert bound(case, prec) < 0.5 * drop, (prec, bound(case, prec), err)
        else:
            assert bound(case, prec) < 0.5 * one, (prec, bound(case, prec), err)


BIDIR_FAULTS = ("fw", "fw_r", "fh", "fh_r", "fih")  # manual_lstm's five places a bidirectional fault can sit


@pytest.mark.parametrize("case", BIDIR_CASES, ids=lambda c: f"D{c.D}-T{c.T}")
def test_bidir_bound_discriminates(case):
    """The same condition for the bidirectional matrix (tests/test_gpu_lstm_bidir_matrix.py): in every precision a case's
    GPU legs run, bound < 1/2 of the smallest error of an fp32 recurrence with a single-plane (bf16) operand, the
    smallest taken over W_hh and h of either direction and the [H, 2H) columns of W_ih.  Measured here at B = 70: cpu32
    4.0e-7 (D = 96) and 1.1e-6 .. 1.6e-6, the smallest single-plane error 1.4e-3 .. 3.9e-3, the smallest dropped-plane
    error 2.2 .. 5.9 x cpu32.  No dropped-plane guarantee is asked (DESIGN.md
    §19); the figures are printed, per place and per channel half."""
    ref = ref64(case)
    m64 = manual_lstm(case, torch.float64)
    for a, b in zip(m64, ref):  # the written-out two-direction loop is torch's bidirectional LSTM
        assert rel_h(a, b) < 1e-12
    err, halves = {}, {}
    for name, n in (("drop", 2), ("one", 1)):
        for place in BIDIR_FAULTS:
            y = manual_lstm(case, torch.float32, **{place: lambda v: planes(v, n)})[0]
            e = rel_h_halves(y, ref[0])
            err[f"{name}_{place}"], halves[f"{name}_{place}"] = e[0], e[1:]
    drop = min(v for k, v in err.items() if k.startswith("drop"))
    one = min(v for k, v in err.items() if k.startswith("one"))
    c32 = cpu32(case)
    print(f"bidir D {case.D} layers {case.layers} T {case.T} B {case.B} whh_scale {case.whh_scale}: max |h| "
          f"{float(ref[0].abs().max()):.3f} cpu32 y {c32[0]:.2e} h_n {c32[1]:.2e} c_n {c32[2]:.2e} " +
          " ".join(f"{k} {v:.2e} (fwd {halves[k][0]:.2e} rev {halves[k][1]:.2e})" for k, v in err.items()) +
          f" drop / cpu32 {drop / max(c32):.1f}; bounds " +
          " ".join(f"{p} {bound(case, p):.2e} (drop = {drop / bound(case, p):.2f} x bound)" for p in bidir_precs(case)))
    assert max(c32) < drop
    for prec in bidir_precs(case):
        assert bound(case, prec) >= max(c32)
        assert bound(case, prec) < 0.5 * one, (prec, bound(case, prec), err)


# ---------------------------------------------------------------------------------------------------------------------
# pack layouts


def _whh(H, seed):
    rng = np.random.default_rng(seed)
    # rows of very different scale: the h3 row scales must follow each row's own maximum
    return (rng.standard_normal((4 * H, H)) / np.sqrt(H) * np.exp2(rng.integers(-6, 7, (4 * H, 1)))).astype(np.float32)


def _seq_index_map(H):
    """lstm_seq_pack: out[g][wave][m-tile][k-step][plane][lane][8]; lane's row m = lane & 15 of the m-tile is unit-major
    (unit 4 mt + (m >> 2) of workgroup g, gate m & 3), its 8 values are k = 32 (wave KS + ks) + 8 (lane >> 4) + j."""
    KS, G = H // 128, H // 8
    g, wv, mt, ks = (np.arange(n) for n in (G, 4, 2, KS))
    lane, j = np.arange(64), np.arange(8)
    m = lane & 15
    row = ((m & 3) * H)[None, None, :] + (g[:, None, None] * 8 + mt[None, :, None] * 4 + (m >> 2)[None, None, :])  # g, mt, lane
    k = (wv[:, None, None, None] * KS + ks[None, :, None, None]) * 32 + (8 * (lane >> 4))[None, None, :, None] + j  # wv, ks, lane, j
    return row[:, None, :, None, :, None], k[None, :, None, :, :, :]  # broadcast to (G, 4, 2, KS, 64, 8)


@pytest.mark.parametrize("H", [1024, 1536])
def test_lstm_seq_pack_layout_x6_wide(H):
    """mode 1 at the two widest persistent kernels: every packed element is the exact three-plane split of the W_hh
    element the index map names (all of them, not a sample)."""
    lib = L.load()
    w = _whh(H, H)
    n = lib.bc_lstm_hh_packed_floats(H, 1)
    assert n * 4 == 4 * H * H * 3 * 2
    out = np.empty(n, np.float32)
    assert lib.bc_lstm_pack_hh(w.ctypes.data, out.ctypes.data, H, 1) == 0
    raw = out.view(np.uint16).reshape(H // 8, 4, 2, H // 128, 3, 64, 8)
    pl = (raw.astype(np.uint32) << 16).view(np.float32)
    row, k = _seq_index_map(H)
    want = w[row, k]
    assert np.array_equal(pl.sum(axis=4, dtype=np.float64), want.astype(np.float64))
    assert np.array_equal(pl[:, :, :, :, 0], torch.from_numpy(want).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize("H", SEQ_H)
def test_lstm_seq_pack_layout_h3(H):
    """mode 3 (and 2, which runs the same recurrence): two fp16 planes of W_hh * S_row in the same order, then 1 / S_row
    of the 4H rows in torch's order; S_row = 2^(14 - e) with 2^e <= max |row| < 2^(e + 1)."""
    lib = L.load()
    w = _whh(H, H + 1)
    n = lib.bc_lstm_hh_packed_floats(H, 3)
    assert n * 4 == 4 * H * H * 2 * 2 + 4 * H * 4 and lib.bc_lstm_hh_packed_floats(H, 2) == n
    out = np.full(n, np.nan, np.float32)
    assert lib.bc_lstm_pack_hh(w.ctypes.data, out.ctypes.data, H, 3) == 0
    nplane = 4 * H * H * 2
    pl = out.view(np.float16)[:nplane].reshape(H // 8, 4, 2, H // 128, 2, 64, 8).astype(np.float32)
    inv = out[nplane // 2:]
    assert inv.shape == (4 * H,)
    amax = np.abs(w).max(axis=1)
    mant, _ = np.frexp(inv)
    assert np.all(mant == 0.5)  # powers of two
    assert np.array_equal(inv, np.exp2(np.floor(np.log2(amax)) - 14).astype(np.float32))
    row, k = _seq_index_map(H)
    want = w[row, k].astype(np.float64)
    got = pl.sum(axis=4, dtype=np.float64) * inv[np.broadcast_to(row, want.shape)]
    assert np.all(np.abs(got - want) <= 2.0 ** -21 * amax[np.broadcast_to(row, want.shape)])
    # plane 0 is the fp16 rounding of the scaled weight, plane 1 of the remainder
    ws = want.astype(np.float32) / inv[np.broadcast_to(row, want.shape)]
    p0 = ws.astype(np.float16).astype(np.float32)
    assert np.array_equal(pl[:, :, :, :, 0], p0)
    assert np.array_equal(pl[:, :, :, :, 1], (ws - p0).astype(np.float16).astype(np.float32))
    if H == 256:
        out2 = np.empty(n, np.float32)
        assert lib.bc_lstm_pack_hh(w.ctypes.data, out2.ctypes.data, H, 2) == 0
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))


@pytest.mark.parametrize("H", [128, 1024])
def test_lstm_pack_hh2_layout(H):
    """mode 0 with H % 128 == 0 (lstm_step_frag_kernel): whh_p2[H / 4][8 waves][NKW / 4][64 lanes][4] with NKW = H / 32;
    lane's row m = lane & 15 is gate-major (gate m >> 2, unit 4 ug + (m & 3)), element i of group q is
    k = 4 (wave NKW + 4 q + i) + (lane >> 4).  A permutation of W_hh."""
    lib = L.load()
    assert H in FRAG_H
    w = np.arange(4 * H * H, dtype=np.float32).reshape(4 * H, H)  # every element names its own place (exact below 2^24)
    n = lib.bc_lstm_hh_packed_floats(H, 0)
    assert n == 4 * H * H
    out = np.full(n, np.nan, np.float32)
    assert lib.bc_lstm_pack_hh(w.ctypes.data, out.ctypes.data, H, 0) == 0
    nkw = H // 32
    P = out.reshape(H // 4, 8, nkw // 4, 64, 4)
    ug, wv, q = (np.arange(s) for s in P.shape[:3])
    lane, i = np.arange(64), np.arange(4)
    m = lane & 15
    row = ((m >> 2) * H + (m & 3))[None, :] + ug[:, None] * 4  # ug, lane
    k = 4 * (wv[:, None, None, None] * nkw + 4 * q[None, :, None, None] + i[None, None, None, :]) + (lane >> 4)[None, None, :, None]
    want = w[row[:, None, None, :, None], k[None]]
    assert np.array_equal(P, want)
    assert np.array_equal(np.sort(out), w.reshape(-1))
