"""The one-launch ResidualUnit matrix on the host (no GPU).

1. The enumeration: the items of tests/test_gpu_resunit_matrix.py are the distinct names bc_resunit_kernel_name gives
   over cfg 100..399, C = 16..272 and d = 1..10 -- 38 today -- and every cfg bc_resunit_select_cfg can return is one
   of them.
2. What the bound (resunit_ref.bound: K[family][output] times the fp32 CPU error of the case) can tell apart: on every
   case of the matrix it stays at or below the tolerance of the hand-picked tests in tests/test_gpu_kernels.py and below
   half the error of an fp32 evaluation on single-plane operands (one bf16 plane for x6, one fp16 plane for h3);
   whether it also stays below half the error of an evaluation that only lost its third bf16 plane is stated, with the
   figures, in test_bound_discriminates.  The definition that computes the degraded evaluations is first checked
   against oracle.bigcodec_oracle.residual_unit in fp64."""
import re

import pytest
import torch

from audiotokenization_amd import _lib as L
from oracle import bigcodec_oracle as O
from resunit_ref import (DEGRADED, ENUM_DILS, FAMILY, K, LOW_PLANE_PROVEN, N_MATRIX_NAMES, SHORT_T, TOL_SUITE, Case, all_cases,
                         bound, branch_over_skip, case_unit, clip_err, cpu32, data, families_of, group_bns, item_cases,
                         item_id, items, names, one_f16, planes, ref64)

# resunit_x6_kernel's (cfg, C) per family, as the tile table and the variant rules stand (32 names)
X6_KERNEL_ITEMS = {
    "x6": {(113, 16), (112, 32), (111, 48), (106, 48), (110, 64), (105, 64), (109, 96), (104, 96), (116, 96), (123, 96),
           (117, 128)},
    "bf16": {(213, 16), (212, 32), (211, 48), (206, 48), (224, 48), (210, 64), (205, 64), (209, 96), (204, 96),
             (216, 96), (223, 96), (217, 128)},
    "h3": {(313, 16), (312, 32), (310, 64), (305, 64), (309, 96), (304, 96), (316, 96), (323, 96), (317, 128)},
}


def test_planes_and_f16():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(planes(v, 3), v)
    assert torch.equal(planes(v, 1), v.to(torch.bfloat16).float())
    e2 = float(((planes(v, 2) - v).abs() / v.abs()).max())
    assert 2.0 ** -19 < e2 <= 2.0 ** -16, e2  # two planes: 16 significant bits
    e1 = float((one_f16(v) - v).abs().max() / v.abs().max())
    assert 2.0 ** -14 < e1 <= 2.0 ** -11, e1  # one fp16 plane of the scaled tensor: 11 significant bits at the maximum


@pytest.mark.parametrize("case", [Case(48, 3, False, 168), Case(96, 9, True, 165), Case(16, 1, False, 5),
                                  Case(192, 9, True, 5)], ids=lambda c: f"C{c.C}-d{c.d}-{'c' if c.causal else 'n'}-T{c.T}")
def test_unit_is_the_oracle(case):
    """resunit_ref.unit in fp64 is oracle.bigcodec_oracle.residual_unit followed by its snake_beta."""
    p = data(case)
    sd = {k: v.double() for k, v in p.sd.items()}
    want = O.residual_unit(p.x.double(), sd, "", case.d, case.causal, False)
    want_act = O.snake_beta(want, p.next_alpha.double(), p.next_beta.double())
    got, got_act = ref64(case)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert clip_err(got, want) < 1e-13 and clip_err(got_act, want_act) < 1e-13


def test_item_list():
    """The matrix's items are the library's own enumeration: 38 distinct names, of which 32 are resunit_x6_kernel
    instantiations on the (cfg, C) of X6_KERNEL_ITEMS, two the 16-wave unit at C = 192, three the strip kernel and one
    resunit_rr_kernel at C = 48 in h3.  A change to the tile table or the variant rules shows here."""
    its = items()
    print(f"{len(its)} items:")
    for it in its:
        print(f"  {item_id(it):18s} BN {it.BN:3d} d {it.dils}  {it.name}")
    assert len(names()) == N_MATRIX_NAMES and len(its) == N_MATRIX_NAMES
    assert len({item_id(it) for it in its}) == len(its)
    x6k = {f: {(it.cfg, it.C) for it in its if it.family == f and it.name.startswith("resunit_x6_kernel<")}
           for f in ("x6", "bf16", "h3")}
    assert x6k == X6_KERNEL_ITEMS
    assert sum(len(v) for v in x6k.values()) == 32
    rest = {item_id(it): (it.name, it.BN, it.dils) for it in its if not it.name.startswith("resunit_x6_kernel<")}
    assert rest == {"x6-122-192": ("resunit_w16_kernel<3, 2, true>", 256, (1, 3, 9)),
                    "bf16-222-192": ("resunit_w16_kernel<1, 2, true>", 256, (1, 3, 9)),
                    "h3-311-48-strip1": ("resunit_strip_kernel<1>", 128, (1,)),
                    "h3-311-48-strip3": ("resunit_strip_kernel<3>", 128, (3,)),
                    "h3-311-48-strip9": ("resunit_strip_kernel<9>", 128, (9,)),
                    "h3-311-48-rr": ("resunit_rr_kernel<48, 4, 1>", 64, (2, 5, 8))}
    for it in its:
        # a name's template arguments carry its precision (P = 3 / 1 / 2 planes for x6 / bf16 / h3)
        if it.name.startswith("resunit_x6_kernel<"):
            P = int(re.match(r"resunit_x6_kernel<\d+, \d+, \d+, \d+, (\d), \d>$", it.name).group(1))
            assert P == {"x6": 3, "bf16": 1, "h3": 2}[it.family], it
            assert it.dils == (1, 3, 9) and it.BN in (64, 128, 256, 512), it
        assert FAMILY[it.cfg // 100] == it.family
        assert it.BN in group_bns(it) and len(item_cases(it)) == (3 * len(group_bns(it)) + 2) * len(it.dils)
        assert max(c.T for c, _ in item_cases(it)) <= 552


def test_select_cfg_returns_items_only():
    """Every cfg bc_resunit_select_cfg returns for C = 16..2048, d = 1..10 and modes 1..3 launches a kernel of the
    matrix; the widths without a one-launch unit and d = 10 give -1."""
    lib = L.load()
    known = names()
    served = set()
    for mode in (1, 2, 3):
        for C in range(16, 2049, 16):
            for d in ENUM_DILS:
                cfg = lib.bc_resunit_select_cfg(C, d, mode)
                if cfg < 0:
                    assert cfg == -1
                    continue
                assert cfg // 100 == mode and C <= 272, (mode, C, d, cfg)
                assert (cfg, C, d) in known[L.resunit_kernel_name(cfg, C, d)], (mode, C, d, cfg)
                served.add((mode, C))
                if d == 10:
                    pytest.fail(f"mode {mode} C {C}: d = 10 selected cfg {cfg}")
    for C in (80, 112, 144, 160, 176, 192):
        assert (3, C) not in served, C
    assert served == {(m, C) for m in (1, 2, 3) for C in (16, 32, 48, 64, 96, 128)} | {(1, 192), (2, 192)}
    assert lib.bc_resunit_select_cfg(48, 3, 0) == -1 and lib.bc_resunit_select_cfg(48, 3, 4) == -1


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: f"C{c.C}-d{c.d}-{'c' if c.causal else 'n'}-T{c.T}")
def test_bound_discriminates(case):
    """Per case: the fp32 CPU error (cpu32), the errors of the fp32 evaluation whose staged input (fx), activated h (fh)
    or weights (fw) were degraded to two bf16 planes (drop), one bf16 plane and one fp16 plane, and the bounds of the
    families that run the case.  A failed line names the figures."""
    ref = ref64(case)
    c32 = cpu32(case)
    # the skip must not hide the branch: in each clip the branch's maximum is at least half the skip's (1.4 to 2.1 times
    # it at the full lengths).  At T = 5 six of the seven taps read padding at d >= 2, the k = 7 output has 1 / sqrt(7)
    # of a full window's deviation and the branch comes to 0.48 .. 1.0 of the skip: 0.4 there (the assertions on the
    # degraded evaluations below hold on those cases all the same)
    assert branch_over_skip(case) >= (0.4 if case.T == SHORT_T else 0.5), branch_over_skip(case)
    err = {}
    for kind, f in DEGRADED.items():
        for hook in ("fx", "fh", "fw"):
            y, ya = case_unit(case, torch.float32, **{hook: f})
            err[kind, hook] = {"raw": clip_err(y, ref[0]), "act": clip_err(ya, ref[1])}
    low = {kind: {o: min(err[kind, h][o] for h in ("fx", "fh", "fw")) for o in ("raw", "act")} for kind in DEGRADED}
    fams = [f for f in families_of(case) if f != "bf16"]
    print(f"C {case.C} d {case.d} causal {case.causal} T {case.T}: branch / skip {branch_over_skip(case):.2f}; " +
          "; ".join(f"{o}: cpu32 {c32[o]:.2e} drop {low['drop'][o]:.2e} ({low['drop'][o] / c32[o]:.1f} x) one_bf16 "
                    f"{low['one_bf16'][o]:.2e} one_f16 {low['one_f16'][o]:.2e}" for o in ("raw", "act")) + "; bounds " +
          " ".join(f"{f} {o} {bound(case, f, o):.2e}" for f in fams for o in ("raw", "act")))
    for o in ("raw", "act"):
        assert c32[o] < low["drop"][o] < 0.01 * low["one_bf16"][o], (o, c32, low)
        for f in fams:
            b = bound(case, f, o)
            assert K[f][o] >= 1.0
            assert b <= TOL_SUITE[o], (f, o, b)
            assert b < 0.5 * low["one_f16" if f == "h3" else "one_bf16"][o], (f, o, b, low)
            if f in LOW_PLANE_PROVEN:
                assert b < 0.5 * low["drop"][o], (f, o, b, low)
