"""The conv launch matrix on the host (no GPU): every x6-family tile (kX6Tiles[0..22]) in its three operand formats and
the 20 fp32 MFMA cfgs, over the shape classes where tiles go wrong.  This module owns the case generator, the support
formulas and the list of kernel instantiations tests/test_gpu_conv_matrix.py must launch, and checks on the CPU that
  - every cfg bc_conv1d_select_cfg / _select_cfg_n returns for Cout = 8..2048 is valid, named, packable, launchable by
    the documented limits, and one of the instantiations the GPU matrix verifies;
  - the limits leave no silent hole (every tile runs the stride-1 classes and the phase-decomposed strided ones);
  - torch's own fp32 CPU conv meets a quarter of the GPU tolerance against fp64 on every matrix case (so the tolerance
    the GPU test applies is not tighter than fp32 arithmetic allows on these inputs);
  - the x6 / bf16 / h3 weight packing at a ragged Cout and Cin is the documented layout."""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiotokenization_amd import _lib as L
from audiotokenization_amd import conv as CV
from oracle import bigcodec_oracle as O

FAMILIES = {"x6": 100, "bf16": 200, "h3": 300}  # cfg base of the 23 shared tiles
PLANES = {"x6": 3, "bf16": 1, "h3": 2}
MODES = {"fp32": 0, "x6": 1, "bf16": 2, "h3": 3}
N_X6_TILES = 23  # kX6Tiles[0..22]; 23 and 24 are the one-launch ResidualUnit's own tiles
MAX_NCOL = 352  # 32 * X6_MAXCOL_ITERS (x6_common.h)
MAX_LDS = 160 * 1024
B = 2
CIN = 44  # one full 32-channel chunk, then a partial chunk with a partial 8-channel group
CLIP_SCALE = (1.0, 37.0)  # a read across the batch stride shows
# the k7 class carries the tanh epilogue: at 37x its arguments reach 200 and fp32 rounding of the argument alone is
# 5e-5 of tanh's range (torch's fp32 CPU conv + tanh: 7x the tolerance), so its second clip is 37x smaller instead
CLIP_SCALE_TANH = (1.0, 1.0 / 37.0)
GUARD = 256  # floats of NaN on each side of x, y, y2 and the residual

# name, K, stride, dilation, phase-decomposed, causal
Cls = collections.namedtuple("Cls", "name K s d phase causal")
CLASSES = [Cls("pw", 1, 1, 1, False, False), Cls("k7", 7, 1, 1, False, False), Cls("k7d9", 7, 1, 9, False, False),
           Cls("k3", 3, 1, 1, False, False), Cls("k2", 2, 1, 1, False, False),
           Cls("s2", 4, 2, 1, False, False), Cls("s4", 8, 4, 1, False, False), Cls("s5", 10, 5, 1, False, False),
           Cls("s2p", 4, 2, 1, True, False), Cls("s4p", 8, 4, 1, True, False), Cls("s5p", 10, 5, 1, True, False),
           Cls("s4p1", 4, 4, 1, True, False),  # a phase conv with a single tap
           Cls("k7d9c", 7, 1, 9, False, True)]  # the causal case: pad_left = (K - 1) d, no right pad
SWEEP_CLASSES = [c for c in CLASSES if not c.phase and not c.causal]  # the library decides about phase cfgs itself

WIDTHS = (24, 40, 72, 80, 104, 128, 136, 160, 320, 576, 640)  # the width sweep through the library's own tile choice
SWEEP_T = (261, 50)  # input lengths
BITID_COUT, BITID_TOUT = 200, ((296, True), (293, False))  # the bit-identity loop's common shape (Tout, aligned input)

# one launch of the matrix: cfg on class cls; x starts xoff floats past an aligned address
Case = collections.namedtuple("Case", "cfg cls Cin Cout Tin Tout pad xoff epis")


def tile_dims(cfg):
    """(MT, WM, NT, WN) of any conv cfg."""
    if cfg % 1000 >= 100:
        mt, nt, wm, wn = L.X6_CFGS[100 + cfg % 100]
        return mt, wm, nt, wn
    return L.CONV_CFGS[cfg][:4]


def tile_bm_bn(cfg):
    mt, wm, nt, wn = tile_dims(cfg)
    return 16 * mt * wm, 16 * nt * wn


def cfg_planes(cfg):
    return {1: 3, 2: 1, 3: 2}[cfg % 1000 // 100]


def x6_lds(cfg, ncol, s):
    """conv1d_x6_kernel.h x6_lds: the P planes of the input tile and two A buffers of one tap."""
    mt, wm, _, _ = tile_dims(cfg)
    p = cfg_planes(cfg)
    bplane = (ncol * (64 if s == 1 else 80) + 15) // 16 * 16
    return p * bplane + 2 * p * wm * mt * 1024


def _choose_pitch(need, s):
    """conv1d.hip choose_pitch: the fp32 kernel's input-tile row pitch (bank-conflict padding)."""
    best, best_conf = need, 1 << 30
    for pad in range(32):
        w = need + pad
        cnt = [0] * 32
        for lane in range(32):
            cnt[((lane >> 4) * w + (lane & 15) * s) & 31] += 1
        if max(cnt) < best_conf:
            best_conf, best = max(cnt), w
        if max(cnt) == 1:
            break
    return best


def supported(cfg, K, s, d):
    """Whether bc_conv1d_fwd runs cfg on a (K, s, d) conv or returns BC_ERR_UNSUPPORTED, by the documented limits:
    x6 family: the input tile's ncol = (BN - 1) s + (K - 1) d + 1 <= 352 columns and x6_lds <= 160 KiB (a phase cfg is
    the stride-1 conv with ceil(K / s) taps); fp32: two stages of (A + B) floats <= 160 KiB."""
    _, bn = tile_bm_bn(cfg)
    if cfg >= 100:
        if cfg >= 1000:
            K, s, d = -(-K // (cfg // 1000)), 1, 1
        ncol = (bn - 1) * s + (K - 1) * d + 1
        return ncol <= MAX_NCOL and x6_lds(cfg, ncol, s) <= MAX_LDS
    _, wm, _, _, bkc = L.CONV_CFGS[cfg]
    pitch = _choose_pitch((bn - 1) * s + (K - 1) * d + 1, s)
    bstage = (bkc * pitch + 63) // 64 * 64
    astage = bkc * K // 4 * wm * 256
    return 2 * (astage + bstage) * 4 <= MAX_LDS


def conv_pad(cls):
    """Padding as test_conv1d computes it; the causal class pads (K - 1) d on the left only."""
    if cls.causal:
        return (cls.K - 1) * cls.d
    return cls.K // 2 * cls.d if cls.s == 1 else cls.s // 2 + cls.s % 2


def in_len(cls, Tout, aligned):
    """An input length that gives Tout outputs; Tin % 4 == 0 for the aligned length where the stride leaves the choice,
    the longest such length (an unused input tail) otherwise."""
    pad = conv_pad(cls)
    lo = (Tout - 1) * cls.s + (cls.K - 1) * cls.d + 1 - (pad if cls.causal else 2 * pad)
    cands = range(lo, lo + cls.s)
    if aligned:
        return next((t for t in cands if t % 4 == 0), lo)
    return next((t for t in reversed(cands) if t % 4 != 0), lo)


def out_len(cls, Tin):
    pad = conv_pad(cls)
    return (Tin + (pad if cls.causal else 2 * pad) - cls.d * (cls.K - 1) - 1) // cls.s + 1


def item_cfgs(family):
    return list(range(20)) if family == "fp32" else [FAMILIES[family] + t for t in range(N_X6_TILES)]


ITEMS = [(f, c) for f in ("x6", "bf16", "h3", "fp32") for c in item_cfgs(f)]


def item_cases(family, cfg0, with_unsupported=True):
    """Every launch of one (precision family, tile) item: Cout = BM + 8 on every class (a second m-group holding half a
    16-row tile), BM - 16 + 5 on the k3 class, Cout = 1 for MT = 1 tiles (the residual-preload epilogue) on the k7 class
    and on the pointwise class, which every cfg runs (the fp32 BKC = 32 cfg of the 16-row tile rejects k7);
    Tout = BN + 40 from an aligned input with Tin % 4 == 0 (16-byte epilogue, 16-byte staging) and BN + 37 from an input
    4 bytes off (scalar epilogue, single-float staging, a ragged last column tile)."""
    bm, bn = tile_bm_bn(cfg0)
    mt = tile_dims(cfg0)[0]
    for cls in CLASSES:
        if cls.phase and family == "fp32":
            continue
        cfg = 1000 * cls.s + cfg0 if cls.phase else cfg0
        if not with_unsupported and not supported(cfg, cls.K, cls.s, cls.d):
            continue
        couts = [bm + 8] + ([bm - 16 + 5] if cls.name == "k3" else [])
        couts += [1] if cls.name in ("k7", "pw") and mt == 1 else []
        epis = ("bias", "nobias", "res_snake") + (("tanh",) if cls.name == "k7" else ())
        for cout in couts:
            for Tout, xoff in ((bn + 40, 0), (bn + 37, 1)):
                Tin = in_len(cls, Tout, xoff == 0)
                assert out_len(cls, Tin) == Tout
                yield Case(cfg, cls, CIN, cout, Tin, Tout, conv_pad(cls), xoff, epis)


def sweep_shapes(Cout):
    """(class, Cin, Cout, Tin) of the width sweep at one width: Cin = Cout at stride 1, Cout / 2 strided."""
    return [(cls, Cout if cls.s == 1 else Cout // 2, Cout, T) for cls in SWEEP_CLASSES for T in SWEEP_T]


def launched_name(cfg, K, s, d, Tin, xoff):
    """The instantiation a launch runs: bc_conv1d_kernel_name's answer, which assumes the launch meets the 16-byte
    staging's conditions (x6_b4_fits: not phase-decomposed, stride 1, Tin % 4 == 0, 16-byte aligned rows); a launch that
    does not runs the same variant with single-float staging."""
    name = L.conv_kernel_name(cfg, K, s, d)
    if cfg < 1000 and s == 1 and Tin % 4 == 0 and xoff % 4 == 0:
        return name
    if name == "conv1d_x6ra_kernel<true>":
        return "conv1d_x6ra_kernel<false>"
    return name[:-len("true>")] + "false>" if name.endswith(", true>") else name


@functools.lru_cache(maxsize=None)
def matrix_names():
    """Distinct kernel instantiations the supported launches of the matrix run: what the GPU test must cover."""
    L.load()
    names = set()
    for family, cfg0 in ITEMS:
        for c in item_cases(family, cfg0, with_unsupported=False):
            names.add(launched_name(c.cfg, c.cls.K, c.cls.s, c.cls.d, c.Tin, c.xoff))
    return frozenset(names)


def tolerance(family, Cin, K):
    """The suite's conv tolerances (test_conv1d, test_h3_tiles_8_vs_16_waves): max |got - want| / max |want|."""
    return 2e-2 if family == "bf16" else 3e-6 * max(1.0, np.sqrt(Cin * K / 64))


class CaseData:
    """Seeded inputs of one conv shape and its fp64 reference per epilogue (computed once, shared by every tile and
    precision that runs the shape): F.conv1d on the weight-normed weight in fp64, then the epilogue in fp64."""

    def __init__(self, cls, Cin, Cout, Tin):
        scale = CLIP_SCALE_TANH if cls.name == "k7" else CLIP_SCALE
        key = repr((tuple(cls), Cin, Cout, Tin)).encode()
        g = torch.Generator().manual_seed(zlib.crc32(key))
        self.cls, self.Cin, self.Cout, self.Tin = cls, Cin, Cout, Tin
        self.pad = conv_pad(cls)
        m = CV.Conv1dWN(Cin, Cout, cls.K, stride=cls.s, dilation=cls.d, padding=self.pad)
        with torch.no_grad():
            m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=g) / np.sqrt(Cin * cls.K))
            m.weight_g.copy_(torch.rand(m.weight_g.shape, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        self.m = m
        self.x = torch.randn(B, Cin, Tin, generator=g) * torch.tensor(scale).reshape(B, 1, 1)
        self.Tout = out_len(cls, Tin)
        self.res = torch.randn(B, Cout, self.Tout, generator=g) * torch.tensor(scale).reshape(B, 1, 1)
        self.alpha = torch.rand(Cout, generator=g) - 0.5  # SnakeBeta parameters (log scale)
        self.beta = torch.rand(Cout, generator=g) - 0.5
        self._want = {}

    def weight(self):
        return O.wn_weight({k: v.detach() for k, v in self.m.state_dict().items()}, "")

    def _conv(self, dtype):
        xp = F.pad(self.x.to(dtype), (self.pad, 0 if self.cls.causal else self.pad))
        return F.conv1d(xp, self.weight().to(dtype), None, stride=self.cls.s, dilation=self.cls.d)

    def want(self, epi, dtype=torch.float64):
        """(raw, activated or None) in dtype (fp64: the reference; fp32: the CPU's own fp32 arithmetic)."""
        k = (epi, dtype)
        if k not in self._want:
            if ("conv", dtype) not in self._want:
                self._want["conv", dtype] = self._conv(dtype)
            y = self._want["conv", dtype]
            if epi != "nobias":
                y = y + self.m.bias.detach().to(dtype).reshape(1, -1, 1)
            act = None
            if epi == "res_snake":
                y = self.res.to(dtype) + y
                act = O.snake_beta(y, self.alpha.to(dtype), self.beta.to(dtype))
            elif epi == "tanh":
                y = torch.tanh(y)
            self._want[k] = (y, act)
        return self._want[k]


@functools.lru_cache(maxsize=None)
def case_data(cls, Cin, Cout, Tin):
    return CaseData(cls, Cin, Cout, Tin)


def clip_rel_err(got, want):
    """max |got - want| / max |want| of the worse clip (the clips differ 37x in scale: a whole-tensor maximum would
    hide the small one)."""
    got, want = got.double(), want.double()
    return max(float((got[b] - want[b]).abs().max() / want[b].abs().max().clamp_min(1e-30)) for b in range(got.shape[0]))


# ---------------------------------------------------------------------------------------------------------------------


def test_matrix_support_has_no_silent_holes():
    """The documented limits admit, for every tile in every precision: the five stride-1 classes, the causal one, every
    phase-decomposed strided class, and the direct strided classes on every BN = 64 tile -- with one exception, a
    hardware limit: the x6 256 x 64 tile at stride 5 (three 26 000-byte planes of the 325-column input tile at the 80-byte
    strided pitch + two A buffers of 3 x 16 KiB = 176 304 bytes of LDS; its h3 and bf16 forms fit).  Every fp32 cfg runs
    the pointwise, k3 and k2 classes, and the BKC = 8 / 4 cfgs of every fp32 tile run every class."""
    lds_exceeded = {("x6", 102, "s5")}
    for family, cfg0 in ITEMS:
        _, bn = tile_bm_bn(cfg0)
        for cls in CLASSES:
            if cls.phase and family == "fp32":
                continue
            if family == "fp32":
                must = cls.name in ("pw", "k3", "k2") or cfg0 % 4 >= 2
            else:
                must = cls.s == 1 or cls.phase or bn == 64
            cfg = 1000 * cls.s + cfg0 if cls.phase else cfg0
            hole = must and not supported(cfg, cls.K, cls.s, cls.d)
            assert hole == ((family, cfg, cls.name) in lds_exceeded), (family, cfg, cls.name)


# the number of distinct instantiations the matrix reaches (a change of the variant rules or the tile table shows here)
N_MATRIX_NAMES = 202


def test_matrix_names():
    names = matrix_names()
    kinds = collections.Counter(n.split("<")[0] for n in names)
    print(f"{len(names)} distinct conv instantiations: {dict(kinds)}")
    assert kinds["conv1d_mfma_kernel"] == 20 and kinds["conv1d_x6ra_kernel"] == 2
    assert len(names) == N_MATRIX_NAMES, sorted(names)
    # every tile of every family launches something in every stride-1 class
    for family, cfg0 in ITEMS:
        have = {c.cls.name for c in item_cases(family, cfg0, with_unsupported=False)}
        need = {"pw", "k3", "k2"} | ({"k7", "k7d9", "k7d9c"} if family != "fp32" or cfg0 % 4 >= 2 else set())
        assert need <= have, (family, cfg0, have)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_selected_cfgs_are_launchable_and_verified(mode):
    """Whatever bc_conv1d_select_cfg (wide launches) and bc_conv1d_select_cfg_n (narrow ones) return for Cout = 8..2048
    is a valid cfg with a kernel name and a packed size, passes the launcher's support limits for the shape, and runs an
    instantiation the GPU matrix checks against fp64."""
    lib = L.load()
    names = matrix_names()
    seen, bad = set(), []
    for cls in SWEEP_CLASSES:
        for Cout in range(8, 2049, 8):
            Cin = Cout if cls.s == 1 else max(Cout // 2, 4)
            args = (Cout, Cin, cls.K, cls.s, cls.d, MODES[mode])
            cfgs = {lib.bc_conv1d_select_cfg(*args)}
            cfgs |= {lib.bc_conv1d_select_cfg_n(*args, b, t) for b, t in ((2, 50), (64, 50), (2, 128), (64, 100), (1, 3))}
            for cfg in cfgs:
                what = (mode, cls.name, Cout, Cin, cfg)
                if cfg < 0 or lib.bc_conv1d_packed_floats(Cout, Cin, cls.K, cfg) < 0:
                    bad.append(("invalid",) + what)
                    continue
                if cfg >= 1000 and (cfg // 1000 != cls.s or cls.d != 1):
                    bad.append(("phase factor",) + what)
                    continue
                if mode == "fp32" and cfg >= 100:
                    bad.append(("fp32 mode left the fp32 kernel",) + what)
                if not supported(cfg, cls.K, cls.s, cls.d):
                    bad.append(("the launcher rejects it",) + what)
                    continue
                name = L.conv_kernel_name(cfg, cls.K, cls.s, cls.d)
                seen.add(name)
                if name not in names:
                    bad.append(("not in the verified matrix: " + name,) + what)
    print(f"{mode}: the select functions reach {len(seen)} instantiations")
    assert not bad, bad[:20]


def _matrix_shapes():
    """Every conv shape the GPU module compares with fp64: the tile matrix, the bit-identity loop's common shape and the
    width sweep."""
    shapes = set()
    for family, cfg0 in ITEMS:
        for c in item_cases(family, cfg0, with_unsupported=False):
            shapes.add((c.cls, c.Cin, c.Cout, c.Tin))
    for cls in CLASSES:
        for Tout, aligned in BITID_TOUT:
            shapes.add((cls, CIN, BITID_COUT, in_len(cls, Tout, aligned)))
    for Cout in WIDTHS:
        shapes.update(sweep_shapes(Cout))
    return sorted(shapes, key=lambda s: (CLASSES.index(s[0]),) + s[1:])


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.name)
def test_fp32_cpu_conv_meets_a_quarter_of_the_tolerance(cls):
    """The condition for using the suite's fp32-class tolerance on the matrix inputs: torch's fp32 CPU conv (and
    epilogue) of every case is within a quarter of it of the fp64 reference, per clip."""
    worst = 0.0
    for c, Cin, Cout, Tin in _matrix_shapes():
        if c != cls:
            continue
        cd = CaseData(c, Cin, Cout, Tin)
        tol = tolerance("fp32", Cin, c.K)
        for epi in ("bias", "nobias", "res_snake") + (("tanh",) if c.name == "k7" else ()):
            (y32, a32), (y64, a64) = cd.want(epi, torch.float32), cd.want(epi)
            e = clip_rel_err(y32, y64)
            worst = max(worst, e / tol)
            assert e <= tol / 4, (c.name, Cout, Tin, epi, e, tol)
            if a64 is not None:
                e = clip_rel_err(a32, a64)
                assert e <= 4 * tol / 4, (c.name, Cout, Tin, epi, "snake", e, tol)
    print(f"{cls.name}: fp32 CPU conv at most {worst:.3f} of the tolerance")


def _bf16_rn(v):
    return torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("cfg,K", [(100, 3), (222, 7), (309, 2), (4113, 8)])
def test_x6_family_pack_layout_ragged(cfg, K):
    """Packed weights of one x6, one bf16 and one h3 tile (and a phase-decomposed one) at Cout = BM + 8, Cin = 44, in the
    [m-group][chunk][tap][plane][m-tile][lane][8] order conv1d_x6.hip documents: rows past Cout and channels past Cin
    are zero in every plane; the three bf16 planes sum back to the fp32 weight exactly, the single bf16 plane is the
    weight rounded to nearest, the two fp16 planes are the split of the row-scaled weight (scale 2^(14 - e) with
    2^e <= max |row| < 2^(e + 1), its inverse stored behind the planes)."""
    lib = L.load()
    bm, _ = tile_bm_bn(cfg)
    mt, wm, _, _ = tile_dims(cfg)
    P, qa = cfg_planes(cfg), mt * wm
    Cout, Cin = bm + 8, CIN
    rng = np.random.default_rng(cfg)
    w = (rng.standard_normal((Cout, Cin, K)) * np.exp(rng.standard_normal((Cout, 1, 1)) * 3)).astype(np.float32)
    n = lib.bc_conv1d_packed_floats(Cout, Cin, K, cfg)
    ps = cfg // 1000
    if ps:  # W'[co][ci * s + r][q] = W[co][ci][q * s + r]
        Kp = -(-K // ps)
        wl = np.zeros((Cout, Cin * ps, Kp), np.float32)
        for k in range(K):
            wl[:, k % ps::ps, k // ps] = w[:, :, k]
    else:
        Kp, wl = K, w
    Cl = wl.shape[1]
    ntm, nch = -(-Cout // bm), -(-Cl // 32)
    assert ntm == 2 and n * 4 == ntm * nch * Kp * P * qa * 1024 + (ntm * bm * 4 if P == 2 else 0)
    out = np.full(n, np.nan, np.float32)
    assert lib.bc_conv1d_pack(w.ctypes.data, out.ctypes.data, Cout, Cin, K, cfg) == 0
    nplane = ntm * nch * Kp * P * qa * 64 * 8
    raw = out.view(np.uint16)[:nplane].reshape(ntm, nch, Kp, P, qa, 64, 8)
    # full weight in the packed index space (zero past the edges)
    full = np.zeros((ntm * bm, nch * 32, Kp), np.float32)
    full[:Cout, :Cl] = wl
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    rows = (np.arange(ntm)[:, None, None, None] * bm + np.arange(qa)[None, :, None, None] * 16 + (lane & 15)[None, None])
    cis = np.arange(nch)[:, None, None] * 32 + (8 * (lane >> 4) + j)[None]
    # want[mg, c, tap, q, lane, j]
    want = full[rows[:, None, None, :, :, :], cis[None, :, None, None, :, :], np.arange(Kp)[None, None, :, None, None, None]]
    if P == 2:
        planes = raw.view(np.float16).astype(np.float32)
        inv = out[nplane // 2:]
        assert inv.shape == (ntm * bm,)
        amax = np.abs(full).max(axis=(1, 2))
        e = np.floor(np.log2(np.where(amax > 0, amax, 2.0 ** 14)))
        scale = np.where(amax > 0, 2.0 ** (14 - e), 1.0).astype(np.float32)
        assert np.array_equal(inv, (1.0 / scale).astype(np.float32))
        ws = want * scale[rows][:, None, None]
        h0 = ws.astype(np.float16).astype(np.float32)
        assert np.array_equal(planes[:, :, :, 0], h0)
        assert np.array_equal(planes[:, :, :, 1], (ws - h0).astype(np.float16).astype(np.float32))
    else:
        planes = (raw.astype(np.uint32) << 16).view(np.float32)
        assert np.array_equal(planes[:, :, :, 0], _bf16_rn(want))
        if P == 3:
            assert np.array_equal(planes.astype(np.float64).sum(axis=3), want.astype(np.float64))
    dead = (rows[:, None, None, :, :, :] >= Cout) | (cis[None, :, None, None, :, :] >= Cl)
    dead = np.broadcast_to(dead[:, :, :, None], raw.shape)
    assert dead.any() and not raw[dead].any()
