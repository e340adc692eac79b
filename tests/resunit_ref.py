"""The one-launch ResidualUnit matrix's items, cases, fp64 definition, metric and bound
(tests/test_resunit_matrix_host.py proves what the bound can tell apart; tests/test_gpu_resunit_matrix.py applies it to
every kernel instantiation of csrc/resunit_x6.hip, resunit_w16.hip and resunit_rr.hip).

The unit is y = x + conv1(snake(conv7_d(snake(x)))).  The case data make the branch 1.4 to 2.1 times the skip (per
clip maximum; 0.48 to 1.0 at T = 5, where most taps read padding), so the skip cannot hide an error of the branch, and
the metric is max |got - want| / max |want| per clip, the worse of the two clips (clip 1 is clip 0's scale / 4: an
error that scales with the batch maximum shows)."""
import collections
import ctypes
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from audiotokenization_amd import _lib as L

Case = collections.namedtuple("Case", "C d causal T")
# One kernel instantiation: family x6 / bf16 / h3, the cfg and width that launch it, its symbol, the tile's column
# count BN and the dilations its cases run at (a strip kernel is compiled for one dilation).
Item = collections.namedtuple("Item", "family cfg C name BN dils")

B = 2
CLIP_SCALE = (1.0, 0.25)
FAMILY = {1: "x6", 2: "bf16", 3: "h3"}
N_MATRIX_NAMES = 38         # distinct instantiations the enumeration finds under the default environment
ENUM_WIDTHS = range(16, 273, 16)
ENUM_DILS = range(1, 11)
DILS = (1, 3, 9)            # where the dilation is a runtime argument
RR_DILS = (2, 5, 8)         # resunit_rr_kernel: the C = 48 h3 dilations the strip kernels do not take
SHORT_T = 5                 # shorter than the 3 d halo at d = 3 and 9
TOL_SUITE = {"raw": 2e-5, "act": 5e-5}  # tests/test_gpu_kernels.py's tolerances: the matrix is never looser
LAYOUTS = ("A", "U", "M")   # A: all aligned; U: x_raw / x_act 4 bytes off; M: y / y2 4 bytes off (T % 4 == 0)
IO_MODES = ("xact", "sin", "sin_dual", "sin_act")  # producer-side x_act; snake on load: plain, y + y2, activated only

# bound = K[family][output] * cpu32(case)[output]: twice the largest ratio (kernel error) / cpu32 measured on the MI355X
# over every item, case, layout and input / output mode of the family, rounded up to one decimal (DESIGN.md has the
# ratios per item; profiles/resunit_matrix_ratios.txt is the log).  Largest measured: x6 raw 1.86 (C = 64), act 2.46
# (C = 16); h3 raw 1.64 (C = 16), act 2.10 (C = 64).
K = {"x6": {"raw": 3.8, "act": 5.0}, "h3": {"raw": 3.3, "act": 4.2}}
# Families whose bound is proved (tests/test_resunit_matrix_host.py) to sit below half the error of an evaluation that
# lost its third bf16 plane ("drop"), on every case.  Neither is: drop is 4.5 to 13 times cpu32 on the raw output of the
# full-length cases (4.1 to 12.5 on the activated one) and 3.8 to 30 (3.1 to 21) at T = 5, so the proof needs K below
# 1.9 (1.55), and twice the measured ratios is 3.3 to 5.0.  The bounds are proved against single-plane operands instead
# (two orders of magnitude above them), and DESIGN.md records what a scratch build with a dropped plane fails.
LOW_PLANE_PROVEN = ()


def _bn(cfg):
    _, NT, _, WN = L.X6_CFGS[100 + cfg % 100]
    return 16 * NT * WN


@functools.lru_cache(maxsize=None)
def names():
    """{kernel name: [(cfg, C, d), ...]} over cfg 100..399, C = 16..272 and d = 1..10, from bc_resunit_kernel_name."""
    lib = L.load()
    out = {}
    buf = ctypes.create_string_buffer(128)
    for cfg in range(100, 400):
        for C in ENUM_WIDTHS:
            for d in ENUM_DILS:
                if lib.bc_resunit_kernel_name(cfg, C, d, buf, 128) >= 0:
                    out.setdefault(buf.value.decode(), []).append((cfg, C, d))
    return out


@functools.lru_cache(maxsize=None)
def items():
    """One Item per distinct kernel name, launched through the cfg bc_resunit_select_cfg picks where that gives the name
    (the C = 48 h3 kernels take any 48-row tile's cfg), else the lowest cfg and width that do."""
    lib = L.load()
    out = []
    for name, where in names().items():
        sel = [w for w in where if lib.bc_resunit_select_cfg(w[1], w[2], w[0] // 100) == w[0]]
        cfg, C, _ = min(sel or where)
        ds = sorted({d for c, w, d in where if (c, w) == (cfg, C)})
        fam = FAMILY[cfg // 100]
        if name.startswith("resunit_strip_kernel"):
            bn, dils = 128, tuple(ds)
        elif name.startswith("resunit_rr_kernel"):
            bn, dils = 64, tuple(d for d in RR_DILS if d in ds)
        else:
            bn, dils = _bn(cfg), tuple(d for d in DILS if d in ds)
        out.append(Item(fam, cfg, C, name, bn, dils))
    return tuple(sorted(out, key=lambda i: (i.cfg // 100, i.C, i.cfg, i.name)))


def item_id(it):
    tag = ""
    if it.name.startswith("resunit_strip_kernel"):
        tag = f"-strip{it.dils[0]}"
    elif it.name.startswith("resunit_rr_kernel"):
        tag = "-rr"
    return f"{it.family}-{it.cfg}-{it.C}{tag}"


def group_bns(it):
    """Column counts of every tile of the item's family and width: an item runs the lengths of all of them, so that
    each bit-identity group (family, C, d, causal, T, layout) holds every cfg of the family and width."""
    return tuple(sorted({i.BN for i in items() if (i.family, i.C) == (it.family, it.C)}))


def item_shapes(it):
    """(T, causal, layout) of an item, per tile width BN of its group (its own included): a full tile plus a ragged
    one, aligned (A) and with the outputs 4 bytes off (M: scalar epilogue, 16-byte staging), the same with causal
    padding and the inputs 4 bytes off (U); and a length below the halo with both paddings."""
    out = []
    for bn in group_bns(it):
        out += [(bn + 40, False, "A"), (bn + 40, False, "M"), (bn + 37, True, "U")]
    return tuple(out) + ((SHORT_T, False, "A"), (SHORT_T, True, "A"))


def item_cases(it):
    """[(Case, layout)] of an item."""
    return [(Case(it.C, d, causal, T), lay) for d in it.dils for T, causal, lay in item_shapes(it)]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(sorted({c for it in items() for c, _ in item_cases(it)}))


def families_of(case):
    """Families whose items run the case."""
    return sorted({it.family for it in items() for c, _ in item_cases(it) if c == case})


# ---------------------------------------------------------------------------------------------------------------------
# data and the definition


@functools.lru_cache(maxsize=None)
def data(case):
    """x (B, C, T) with the clips scaled 1 and 0.25, the unit's state dict under ResidualUnit's names (v7 ~ N / sqrt(7 C),
    v1 ~ N / sqrt(C), g ~ U(0.5, 1.5), biases 0.1 N, Snake log-parameters U(-0.5, 0.5)) and the next Snake's alpha / beta.
    Shared and never written."""
    C, d, causal, T = case
    g = torch.Generator().manual_seed(zlib.crc32(repr((C, d, bool(causal), T)).encode()))
    randn = lambda *s: torch.randn(*s, generator=g)
    uni = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    p7 = "block.1.conv." if causal else "block.1."
    sd = {p7 + "weight_v": randn(C, C, 7) / np.sqrt(7 * C), p7 + "weight_g": uni(0.5, 1.5, C, 1, 1),
          p7 + "bias": 0.1 * randn(C),
          "block.3.weight_v": randn(C, C, 1) / np.sqrt(C), "block.3.weight_g": uni(0.5, 1.5, C, 1, 1),
          "block.3.bias": 0.1 * randn(C)}
    for k in ("block.0.act.", "block.2.act."):
        sd[k + "alpha"] = uni(-0.5, 0.5, C)
        sd[k + "beta"] = uni(-0.5, 0.5, C)
    x = randn(B, C, T) * torch.tensor(CLIP_SCALE).view(B, 1, 1)
    return types.SimpleNamespace(x=x, sd=sd, p7=p7, next_alpha=uni(-0.5, 0.5, C), next_beta=uni(-0.5, 0.5, C))


def snake(x, alpha, beta):
    """SnakeBeta with log-scale parameters: x + 1 / (exp(beta) + 1e-9) * sin(x * exp(alpha))**2."""
    a, b = torch.exp(alpha).view(1, -1, 1), torch.exp(beta).view(1, -1, 1)
    return x + 1.0 / (b + 1e-9) * torch.sin(x * a) ** 2


def unit(x, params, d, causal, dtype, fx=None, fh=None, fw=None):
    """The unit in plain torch in `dtype`: (raw output, next Snake of it).  fx / fh / fw replace the staged activated
    input, the activated h and both folded weights (the degraded evaluations of the host test)."""
    ident = lambda v: v
    fx, fh, fw = fx or ident, fh or ident, fw or ident
    sd = {k: v.to(dtype) for k, v in params.sd.items()}
    x = x.to(dtype)

    def wn(p):
        v, g = sd[p + "weight_v"], sd[p + "weight_g"]
        return g * v / v.reshape(v.shape[0], -1).norm(dim=1).view(-1, 1, 1)

    xa = fx(snake(x, sd["block.0.act.alpha"], sd["block.0.act.beta"]))
    pad = (6 * d, 0) if causal else (3 * d, 3 * d)
    h = F.conv1d(F.pad(xa, pad), fw(wn(params.p7)), sd[params.p7 + "bias"], dilation=d)
    ha = fh(snake(h, sd["block.2.act.alpha"], sd["block.2.act.beta"]))
    y = x + F.conv1d(ha, fw(wn("block.3.")), sd["block.3.bias"])
    return y, snake(y, params.next_alpha.to(dtype), params.next_beta.to(dtype))


def case_unit(case, dtype, **hooks):
    p = data(case)
    with torch.no_grad():
        return unit(p.x, p, case.d, case.causal, dtype, **hooks)


@functools.lru_cache(maxsize=None)
def ref64(case):
    """The reference: (raw, activated) in float64, one per case, shared by every cfg, precision, layout and mode."""
    return case_unit(case, torch.float64)


def planes(v, n):
    """The sum of the first n bf16 planes of v (3 planes hold an fp32 value exactly: the x6 operand)."""
    r, s = v.clone(), torch.zeros_like(v)
    for _ in range(n):
        p = r.to(torch.bfloat16).to(v.dtype)
        s, r = s + p, r - p
    return s


def one_f16(v):
    """One fp16 plane of the tensor scaled by its maximum (an h3 operand that lost its second plane)."""
    s = v.abs().max().clamp_min(1e-30)
    return (v / s).to(torch.float16).to(v.dtype) * s


DEGRADED = {"drop": lambda v: planes(v, 2), "one_bf16": lambda v: planes(v, 1), "one_f16": one_f16}


def clip_err(got, want):
    """max |got - want| / max |want| per clip, the worse clip."""
    got, want = got.double(), want.double()
    e = (got - want).abs().flatten(1).max(dim=1)[0] / want.abs().flatten(1).max(dim=1)[0].clamp_min(1e-30)
    return float(e.max())


def worst(got, want):
    d = (got.double() - want.double()).abs()
    i = tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))
    return f"worst at clip {i[0]}, channel {i[1]}, column {i[2]}: got {float(got[i])!r}, want {float(want[i])!r}"


@functools.lru_cache(maxsize=None)
def cpu32(case):
    """{"raw", "act"}: error of torch's fp32 CPU arithmetic on the case against fp64."""
    y, ya = case_unit(case, torch.float32)
    r = ref64(case)
    return {"raw": clip_err(y, r[0]), "act": clip_err(ya, r[1])}


def bound(case, family, output):
    """The largest clip_err an x6 / h3 kernel may show on the case's raw ("raw") or activated ("act") output."""
    return K[family][output] * cpu32(case)[output]


def branch_over_skip(case):
    """min over the clips of max |y - x| / max |x|."""
    x, y = data(case).x.double(), ref64(case)[0]
    return float(((y - x).abs().flatten(1).max(dim=1)[0] / x.abs().flatten(1).max(dim=1)[0]).min())
