"""The transposed-conv and anti-aliased-Snake matrices on the host (no GPU).  This module owns the case tables of
tests/test_gpu_convt_matrix.py and tests/test_gpu_aa_matrix.py and checks on the CPU that
  - the polyphase restatement (tests/convt_ref.py) equals F.conv_transpose1d in float64 on every table entry, and its
    phases cover every output exactly once;
  - the library's host functions (bc_convT1d_phase_taps, bc_convT1d_workspace_floats, bc_aa_snake_out_len) and the
    Python side (ConvTranspose1dWN.out_len, the weight slicing of ConvTranspose1dWN.prepared) agree with it;
  - the table's refused geometries are exactly those with padding > s (Kp - 1).

Geometries are (s, K, p, output_padding, crop).  Each runs at widths (44, 24) (one full 32-channel chunk and a partial
one with a partial 8-channel group), (96, 200) and (384, 192), the three presets also at (1536, 768) with Tin <= 31, on
input lengths 1, 2, 3, 4, 5, 31, 64, 65, the narrow-launch boundary 128 / 129 and BN + 5 (a second column tile of the
tile the library chooses for the width in the family).  Together: Tout % 4 == 0 and != 0 (the interleave's two store
branches), Tin % 4 == 0 and != 0.  Two geometries are added to the issue's table: a crop of 8 at s = 5, the only one
with phases that have no output at all (Tout = 2 at Tin = 1; every other geometry has Tout >= s at every length), and
K = 10 at s = 2 (five taps per phase: the bf16 kernels stage 16 bytes at a time only from four taps per K-step on)."""
import collections
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import convt_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import conv as CV
from audiotokenization_amd import modules as M
from test_conv_matrix_host import B, CLIP_SCALE, FAMILIES, MODES, tile_bm_bn

Geom = collections.namedtuple("Geom", "s K p opad crop")
GEOMS = [Geom(*g) for g in (
    (2, 4, 1, 0, 0), (4, 8, 2, 0, 0), (5, 10, 3, 1, 0),   # the decoder presets
    (2, 4, 0, 0, 2), (4, 8, 0, 0, 4), (5, 10, 0, 0, 5),   # their causal forms
    (1, 1, 0, 0, 0), (2, 2, 0, 0, 0), (4, 4, 0, 0, 0),    # one tap per phase: the pointwise kernel variants
    (2, 6, 2, 0, 0),                                      # three taps
    (2, 5, 1, 0, 0), (4, 6, 1, 0, 0),                     # K % s != 0: a zero-filled tap
    (3, 6, 2, 1, 0),                                      # odd stride with output padding
    (8, 16, 4, 0, 0), (16, 32, 8, 0, 0),                  # 16: the last entry of the interleave's table
    (17, 34, 9, 1, 0),                                    # 17: beyond it, the direct path only
    (2, 4, 2, 0, 0),                                      # the largest supported padding, p = s (Kp - 1)
    (5, 10, 0, 0, 8),                                     # Tout = 2 < s at Tin = 1: three phases without any output
    (2, 10, 4, 0, 0))]                                    # five taps: bf16's multi-tap variant with 16-byte staging
PRESETS = GEOMS[:3]
REFUSED = [Geom(2, 4, 3, 0, 0), Geom(4, 4, 1, 0, 0)]
MAX_WS_STRIDE = 16  # bc_internal.h CONVT_MAX_STRIDE
BASE_T = (1, 2, 3, 4, 5, 31, 64, 65)
WIDTHS = ((44, 24), (96, 200), (384, 192))
WIDE = (1536, 768)  # the presets only, Tin <= 31 (its float64 reference is the slow part)
SUBSET_T, SUBSET_W = (4, 5, 65), (44, 24)  # misaligned y, the registered op
TILE_T = 64  # narrow-launch tile against the default tile
FAMILY_NAMES = ("fp32", "x6", "bf16", "h3")
ITEMS = [(f, g) for f in FAMILY_NAMES for g in GEOMS]


def geom_id(g):
    return "s{}k{}p{}o{}c{}".format(*g)


def default_cfg(family, Cin, Cout, Kp):
    """The tile of the phase convs at Tin > 128 (ConvTranspose1dWN.phase_cfg())."""
    return L.conv_cfg(Cout, Cin, Kp, 1, 1, MODES[family])


def launch_cfg(family, Cin, Cout, Kp, Tin):
    """ConvTranspose1dWN.phase_cfg(B, Tin): the narrow-launch choice up to 128 columns."""
    cfg = default_cfg(family, Cin, Cout, Kp)
    if 0 < Tin <= 128:
        n = L.load().bc_conv1d_select_cfg_n(Cout, Cin, Kp, 1, 1, MODES[family], B, Tin)
        cfg = n if n >= 0 else cfg
    return cfg


def lengths(family, g, Cin, Cout):
    """Input lengths of one (family, geometry, width), those without any output dropped."""
    if (Cin, Cout) == WIDE:
        ts = [t for t in BASE_T if t <= 31]
    else:
        bn = tile_bm_bn(default_cfg(family, Cin, Cout, R.phase_taps(g.K, g.s)))[1]
        ts = sorted(set(BASE_T + (128, 129, bn + 5)))
    return [t for t in ts if R.out_len(t, *g) > 0]


def widths(g):
    return WIDTHS + ((WIDE,) if g in PRESETS else ())


def item_cases(family, g):
    for Cin, Cout in widths(g):
        for Tin in lengths(family, g, Cin, Cout):
            yield Cin, Cout, Tin


class CaseData:
    """Seeded module, inputs and float64 references of one (geometry, width, length), shared by the families."""

    def __init__(self, g, Cin, Cout, Tin):
        gen = torch.Generator().manual_seed(zlib.crc32(repr((tuple(g), Cin, Cout, Tin)).encode()))
        Kp = R.phase_taps(g.K, g.s)
        m = CV.ConvTranspose1dWN(Cin, Cout, g.K, g.s, padding=g.p, output_padding=g.opad)
        m.causal_crop = g.crop
        with torch.no_grad():
            m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=gen) / np.sqrt(Cin * Kp))
            m.weight_g.copy_((torch.rand(m.weight_g.shape, generator=gen) + 0.5) * np.sqrt(Cout / Cin))
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        self.m, self.g, self.Cin, self.Cout, self.Tin, self.Kp = m, g, Cin, Cout, Tin, Kp
        self.x = torch.randn(B, Cin, Tin, generator=gen) * torch.tensor(CLIP_SCALE).reshape(B, 1, 1)
        self.Tout = R.out_len(Tin, *g)
        snk = M.SnakeBeta(Cout, alpha_logscale=True)
        with torch.no_grad():
            snk.alpha.copy_(torch.rand(Cout, generator=gen) - 0.5)
            snk.beta.copy_(torch.rand(Cout, generator=gen) - 0.5)
        self.snake = snk
        self._want = {}

    def wn(self):
        return (self.m.weight_v.detach(), self.m.weight_g.detach())

    def want(self, bias=True, dtype=torch.float64):
        """(raw, Snake of raw) of the transposed conv in dtype."""
        k = (bias, dtype)
        if k not in self._want:
            g = self.g
            y = R.convt(self.x.to(dtype), self.wn(), self.m.bias.detach() if bias else None, g.s, g.p, g.opad, g.crop)
            self._want[k] = (y, R.snake(y, *self.snake._host_coeffs()))
        return self._want[k]


@functools.lru_cache(maxsize=None)
def case_data(g, Cin, Cout, Tin):
    return CaseData(g, Cin, Cout, Tin)


# ---- the anti-aliased Snake's cases ----------------------------------------------------------------------------------
AA_B, AA_C = 3, 5
AA_FIXED_T = (1, 2, 5, 6, 127, 128, 129, 255, 256, 257, 511, 513)
AA_ADDED = ((16, 16, 32, 32), (1, 16, 1, 33), (3, 2, 256, 7), (2, 3, 4, 256))
AA_TARGETS = (1, 255, 256, 257, 513)  # output lengths around the 256-output tile's edges
AA_REFUSED = ((2, 2, 257, 12), (2, 2, 12, 257), (17, 2, 34, 12), (2, 17, 12, 34), (4, 2, 3, 12))  # (ru, rd, ku, kd)


# Cases whose float32 yardstick is pooled over redraws (aa_own): the fixed kernel at T = 1 has five outputs per clip,
# and the largest of five float32 rounding errors is too noisy a yardstick -- on the MI355X the kernel's error on the
# 37 x clip is 7.68e-5 (2.6 float32 ulp of max |ref| = 248: rounding of the Snake's argument), 4.88 times the restatement's
# 1.57e-5 on the same five outputs, while the restatement's own error over 16 draws of the case reaches 4.76e-5.
AA_POOLED = {("fixed", 1): 16}


def aa_golden_sets():
    """(ru, rd, ku, kd) of tests/golden/aa_activation_ratios.npz, the default tap counts (Activation1d) filled in."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aa_activation_ratios.npz"))
    sets = []
    for ru, rd, ku, kd in json.loads(str(d["meta"]))["cases"]:
        sets.append((ru, rd, M.UpSample1d(ru, ku).kernel_size, M.DownSample1d(rd, kd).kernel_size))
    return tuple(sets)


def aa_sets():
    return aa_golden_sets() + AA_ADDED


def aa_lengths(ru, rd, kd):
    """T = 1 and, per target output length, the shortest input whose output reaches it (the output length grows in
    steps of ru / rd or 1: where the target itself is skipped, the next length above it)."""
    ts = {1}
    for want in AA_TARGETS:
        ts.add(next(t for t in range(1, 20000) if R.aa_out_len(t, ru, rd, kd) >= want))
    return sorted(ts)


def aa_filters(ru, rd, ku, kd):
    """The float32 filters as UpSample1d / DownSample1d build them."""
    return (M.kaiser_sinc_filter1d(0.5 / ru, 0.6 / ru, ku).reshape(-1).contiguous(),
            M.kaiser_sinc_filter1d(0.5 / rd, 0.6 / rd, kd).reshape(-1).contiguous())


def aa_inputs(key, T):
    """(x, alpha_exp, inv_beta): x = 3 randn with clip 1 = 37 x clip 0, alpha = exp(N(0, 0.5)), beta likewise, as the
    kernel receives them (SnakeBeta.coeffs)."""
    gen = torch.Generator().manual_seed(zlib.crc32(repr((key, T)).encode()))
    x = 3 * torch.randn(AA_B, AA_C, T, generator=gen)
    x[1] = 37 * x[0]
    snk = M.SnakeBeta(AA_C, alpha_logscale=True)
    with torch.no_grad():
        snk.alpha.copy_(0.5 * torch.randn(AA_C, generator=gen))
        snk.beta.copy_(0.5 * torch.randn(AA_C, generator=gen))
    a, ib = snk._host_coeffs()
    return x, a.contiguous(), ib.contiguous()


def aa_own(key, T, fu, fd, ru, rd):
    """Per clip, max |ref32 - ref64| of the restatement on the case's inputs: the yardstick of the activation's bound.
    For a case in AA_POOLED the maximum also runs over that many draws of the same case (other seeds), which makes it
    a maximum over as many outputs as the longer cases have; it never depends on a kernel's output."""
    own = [0.0] * AA_B
    for j in range(AA_POOLED.get((key, T), 1)):
        x, a, ib = aa_inputs(key if j == 0 else (key, j), T)
        d = (R.aa_act(x, a, ib, fu, fd, ru, rd).double() - R.aa_act(x.double(), a, ib, fu, fd, ru, rd)).abs()
        own = [max(o, float(d[b].max())) for b, o in enumerate(own)]
    return own


# ---------------------------------------------------------------------------------------------------------------------


def _all_entries(g):
    """Every (Cin, Cout, Tin) of a geometry over the four families."""
    return sorted({c for f in FAMILY_NAMES for c in item_cases(f, g)})


@pytest.mark.parametrize("g", GEOMS, ids=geom_id)
def test_polyphase_equals_conv_transpose(g):
    """convt_polyphase = convt in float64 to 1e-12 of max |ref| on every table entry (with and without bias), and every
    output position belongs to exactly one (phase, q)."""
    n = 0
    for Cin, Cout, Tin in _all_entries(g):
        cd = case_data(g, Cin, Cout, Tin)
        for bias in (True, False):
            want = cd.want(bias)[0]
            got, ph = R.convt_polyphase(cd.x.double(), cd.wn(), cd.m.bias.detach() if bias else None, g.s, g.p, g.opad,
                                        g.crop)
            assert got.shape == want.shape == (B, Cout, cd.Tout)
            assert not torch.isnan(got).any(), (g, Cin, Cout, Tin)
            err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
            assert err <= 1e-12, (g, Cin, Cout, Tin, bias, err)
        hits = np.zeros(cd.Tout, int)
        for r, (q_lo, n_out) in enumerate(ph):
            t = g.s * (q_lo + np.arange(n_out)) - g.p + r
            assert n_out == 0 or (t[0] >= 0 and t[-1] < cd.Tout)
            hits[t] += 1
        assert (hits == 1).all(), (g, Tin, hits)
        n += 1
    assert n >= 3 * len(BASE_T) - 3


def test_table_reaches_the_edges():
    """What the docstring promises of the lengths: both interleave store branches, both staging alignments, a phase
    without any output, at least one second column tile per width."""
    for g in GEOMS:
        touts = [R.out_len(t, *g) for _, _, t in _all_entries(g)]
        assert any(t % 4 == 0 for t in touts) or g == Geom(2, 5, 1, 0, 0), g  # (Tout = 2 Tin + 1 there)
        assert any(t % 4 for t in touts) or g.s % 4 == 0, g  # (Tout = s Tin at the table's strides 4, 8, 16)
        tins = {t for _, _, t in _all_entries(g)}
        assert {4, 64, 128} <= tins and {5, 65, 129} <= tins
    empty = [g for g in GEOMS for _, _, t in _all_entries(g)
             if any(n == 0 for _, n in R.phases(R.out_len(t, *g), g.s, g.p))]
    assert set(empty) == {Geom(5, 10, 0, 0, 8)}  # every other geometry has Tout >= s at every length
    for f in FAMILY_NAMES:
        for Cin, Cout in WIDTHS:
            bn = tile_bm_bn(default_cfg(f, Cin, Cout, 2))[1]
            assert bn + 5 in lengths(f, GEOMS[0], Cin, Cout)
            if f != "fp32":
                assert FAMILIES[f] <= default_cfg(f, Cin, Cout, 2) < FAMILIES[f] + 100  # a tile of the family


def test_host_functions_match_the_restatement():
    """bc_convT1d_phase_taps, bc_convT1d_workspace_floats (single and dual), ConvTranspose1dWN.out_len."""
    lib = L.load()
    for g in GEOMS + REFUSED:
        Kp = R.phase_taps(g.K, g.s)
        assert lib.bc_convT1d_phase_taps(g.K, g.s) == Kp
        for Cin, Cout, Tin in (_all_entries(g) if g in GEOMS else [(44, 24, 5)]):
            m = case_data(g, Cin, Cout, Tin).m
            Tout = R.out_len(Tin, *g)
            assert m.out_len(Tin) == Tout
            if g.crop == g.s and g.p == 0 and g.opad == 0:
                assert CV.CausalConvTranspose1d(4, 4, g.K, g.s).conv.out_len(Tin) == Tout
            for dual in (0, 1):
                n = lib.bc_convT1d_workspace_floats(B, Cout, Tout, g.K, g.s, g.p, dual)
                if g.s > MAX_WS_STRIDE:
                    assert n == -1
                else:
                    assert n == R.workspace_floats(B, Cout, Tout, g.s, g.p, dual), (g, Cout, Tin, dual)
                    assert n % 4 == 0 and n >= B * Cout * Tout * (1 + dual)


def test_refused_set_is_padding_beyond_the_first_phase():
    """The table's refused geometries are exactly those with p > s (Kp - 1); (2, 4, 2) is the boundary that runs."""
    for g in GEOMS + REFUSED:
        assert R.supported(g.s, g.K, g.p) == (g not in REFUSED), g
        assert R.supported(g.s, g.K, g.p) == (g.p <= g.s * (R.phase_taps(g.K, g.s) - 1))
    assert Geom(2, 4, 2, 0, 0) in GEOMS
    for g in REFUSED:  # p < K in both: "padding >= K" is not the condition
        assert g.p < g.K


@pytest.mark.parametrize("g", [GEOMS[2], GEOMS[10], GEOMS[11], GEOMS[15], GEOMS[8]], ids=geom_id)
def test_prepared_slices_the_phases_as_the_restatement(g):
    """ConvTranspose1dWN.prepared packs, per phase, the stride-1 weight k = r + s (Kp - 1 - jp) (zero past K)."""
    lib = L.load()
    cd = case_data(g, 44, 24, 5)
    cfg = 14  # an fp32 layout: the packed floats are the weights themselves
    phases, _, bias, got_cfg = cd.m.prepared("cpu", cfg)
    assert got_cfg == cfg and len(phases) == g.s and torch.equal(bias, cd.m.bias.detach())
    w = cd.m.folded_weight()
    assert torch.allclose(w.double(), R.wn_weight(*cd.wn(), torch.float64), rtol=1e-6, atol=0)
    n = lib.bc_conv1d_packed_floats(24, 44, cd.Kp, cfg)
    distinct = set()
    for r in range(g.s):
        wr = R.phase_weight(w, r, g.s).contiguous()
        assert g.K % g.s == 0 or r < g.K % g.s or not wr[:, :, 0].any()  # the zero-filled tap is the first one
        want = np.full(n, np.nan, np.float32)
        assert lib.bc_conv1d_pack(wr.numpy().ctypes.data, want.ctypes.data, 24, 44, cd.Kp, cfg) == 0
        assert np.array_equal(phases[r].numpy(), want), (g, r)
        distinct.add(want.tobytes())
    assert len(distinct) == g.s


def test_aa_out_len_and_lengths():
    """bc_aa_snake_out_len = the restatement's length = the length of aa_act's output, on every activation case; each
    set reaches both sides of the 256-output tile edge and a third tile."""
    lib = L.load()
    assert len(aa_golden_sets()) == 6 and (2, 2, 12, 12) not in aa_sets()
    for T in AA_FIXED_T:
        assert lib.bc_aa_snake_out_len(T, 2, 2, 12) == R.aa_out_len(T, 2, 2, 12) == T
    for ru, rd, ku, kd in aa_sets():
        fu, fd = aa_filters(ru, rd, ku, kd)
        assert fu.numel() == ku and fd.numel() == kd
        outs = []
        for T in aa_lengths(ru, rd, kd):
            n = lib.bc_aa_snake_out_len(T, ru, rd, kd)
            x, a, ib = aa_inputs((ru, rd, ku, kd), T)
            assert n == R.aa_out_len(T, ru, rd, kd) == R.aa_act(x.double(), a, ib, fu, fd, ru, rd).shape[-1]
            outs.append(n)
        assert outs[0] >= 1 and any(254 <= n <= 256 for n in outs) and any(257 <= n <= 272 for n in outs), outs
        assert max(outs) >= 513


def test_aa_pooled_yardstick():
    """aa_own of a pooled case contains the case's own draw, stays float32-class (below 1e-6 of the clip's scale), and
    only the listed case is pooled."""
    fu, fd = aa_filters(2, 2, 12, 12)
    assert set(AA_POOLED) == {("fixed", 1)}
    x, a, ib = aa_inputs("fixed", 1)
    ref64 = R.aa_act(x.double(), a, ib, fu, fd, 2, 2)
    single = [float((R.aa_act(x, a, ib, fu, fd, 2, 2)[b].double() - ref64[b]).abs().max()) for b in range(AA_B)]
    pooled = aa_own("fixed", 1, fu, fd, 2, 2)
    assert all(p >= s1 for p, s1 in zip(pooled, single))
    assert all(p <= 1e-6 * float(ref64[b].abs().max()) for b, p in enumerate(pooled)), pooled
    x2, a2, b2 = aa_inputs("fixed", 2)
    d2 = (R.aa_act(x2, a2, b2, fu, fd, 2, 2).double() - R.aa_act(x2.double(), a2, b2, fu, fd, 2, 2)).abs()
    assert aa_own("fixed", 2, fu, fd, 2, 2) == [float(d2[b].max()) for b in range(AA_B)]


def test_aa_restatement_matches_the_oracle():
    """Where oracle.upsample2 / downsample2 are defined (a right crop > 0), aa_act is the same computation."""
    from oracle import bigcodec_oracle as O

    for ru, rd, ku, kd in aa_golden_sets():
        fu, fd = aa_filters(ru, rd, ku, kd)
        x, a, ib = aa_inputs((ru, rd, ku, kd), 37)
        xd = x.double()
        want = O.downsample2(R.snake(O.upsample2(xd, fu.double().reshape(1, 1, -1), ru), a, ib),
                             fd.double().reshape(1, 1, -1), rd)
        got = R.aa_act(xd, a, ib, fu, fd, ru, rd)
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
