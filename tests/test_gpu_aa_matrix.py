"""The anti-aliased Snake (aa_snake_kernel, aa_snake_gen_kernel) against float64 on the MI355X.

Raw calls bc_aa_snake_fwd / bc_aa_snake_fwd_ex with x, the filters and the NaN-initialised output between NaN guard
bands, B = 3, C = 5, x = 3 randn with the second clip 37 times the first, alpha = exp(N(0, 0.5)), beta likewise (Snake
arguments far below the sinf fallback of test_snake).  Fixed kernel: T on both sides of the 256-output tile's edges.
General kernel: the six ratio sets of tests/golden/aa_activation_ratios.npz and four more -- the largest ratios, a
one-tap up filter with the largest down ratio, 256 taps on either side -- each at input lengths whose output lengths
are 1 and the first at or above 255, 256, 257 and 513 (tests/test_convt_matrix_host.py aa_lengths).

Bound (the rule of tests/test_gpu_conformer_ops.py), per clip: max |got - ref64| <= min(4 x max |ref32 - ref64|,
1e-4 x max |ref64|), ref32 / ref64 the restatement tests/convt_ref.py aa_act in float32 / float64 on the kernel's own
operands.  One case takes its yardstick max |ref32 - ref64| over 16 draws of the case instead of its own five outputs
per clip (tests/test_convt_matrix_host.py AA_POOLED: the fixed kernel at T = 1, measured err / own 4.88 against the
single draw, 1.61 against the pooled one).  A NaN left in the output or a touched band fails the case."""
import pytest
import torch

import convt_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import modules as M
from helpers import assert_close_rel
from test_convt_matrix_host import (AA_FIXED_T, AA_REFUSED, aa_filters, aa_golden_sets, aa_inputs, aa_lengths, aa_own,
                                    aa_sets)
from test_gpu_conv_matrix import _guarded, _guards_intact, _sync, _untouched

pytestmark = pytest.mark.gpu

WORST = [0.0, ""]  # the largest err / (float32 restatement's error) of the module and its case


def _st():
    return torch.cuda.current_stream().cuda_stream


def _run(dev, x, a, ib, fu, fd, ru, rd, fixed_entry):
    """The raw call on guarded operands; returns (return code, guarded output, guarded inputs)."""
    lib = L.load()
    Bn, C, T = x.shape
    ku, kd = fu.numel(), fd.numel()
    Tout = lib.bc_aa_snake_out_len(T, ru, rd, kd)
    ins = [_guarded(dev, tuple(t.shape), 0, t) for t in (x, a, ib, fu, fd)]
    yg = _guarded(dev, (Bn, C, max(Tout, 1)))
    p = [g[1].data_ptr() for g in ins] + [yg[1].data_ptr()]
    if fixed_entry:
        rc = lib.bc_aa_snake_fwd(*p, Bn, C, T, _st())
    else:
        rc = lib.bc_aa_snake_fwd_ex(*p, Bn, C, T, ru, ku, rd, kd, _st())
    _sync(f"aa snake ru {ru} rd {rd} ku {ku} kd {kd} T {T}")
    return rc, yg, ins


def _check(what, yg, ins, key, x, a, ib, fu, fd, ru, rd, fails):
    ref64 = R.aa_act(x.double(), a, ib, fu, fd, ru, rd)
    owns = aa_own(key, x.shape[-1], fu, fd, ru, rd)
    got = yg[1].cpu()
    if tuple(got.shape) != tuple(ref64.shape):
        fails.append(f"{what}: output length {got.shape[-1]}, the restatement's {ref64.shape[-1]}")
        return
    if not _guards_intact(yg) or not all(_guards_intact(g) for g in ins):
        fails.append(f"{what}: a guard band was written")
    if bool(torch.isnan(got).any()):
        fails.append(f"{what}: {int(torch.isnan(got).sum())} NaN of {got.numel()} left in the output")
        return
    for b in range(got.shape[0]):
        scale = float(ref64[b].abs().max())
        own = owns[b]
        bound = min(4.0 * own, 1e-4 * scale)
        d = (got[b].double() - ref64[b]).abs()
        err = float(d.max())
        ratio = err / own if own > 0 else (0.0 if err == 0 else float("inf"))
        print(f"{what} clip {b}: err {err:.3e}, float32 restatement {own:.3e} (err / own {ratio:.2f}), "
              f"bound {bound:.3e}, max|ref| {scale:.3e}")
        if ratio > WORST[0]:
            WORST[0], WORST[1] = ratio, f"{what} clip {b}"
        if not err <= bound:
            t = int(d.max(0)[0].argmax())
            fails.append(f"{what} clip {b}: err {err:.3e} > {bound:.3e} (err / own {ratio:.2f}), worst at t = {t} "
                         f"(tile {t // 256}, position {t % 256})")


@pytest.mark.parametrize("entry", ["fwd", "fwd_ex"])
def test_fixed_kernel(dev, entry):
    """aa_snake_kernel (2x / 2x, 12 taps) through both entry points."""
    fu, fd = aa_filters(2, 2, 12, 12)
    fails = []
    for T in AA_FIXED_T:
        x, a, ib = aa_inputs("fixed", T)
        rc, yg, ins = _run(dev, x, a, ib, fu, fd, 2, 2, entry == "fwd")
        what = f"fixed {entry} T {T}"
        if rc != 0:
            fails.append(f"{what}: return code {rc}")
            continue
        _check(what, yg, ins, "fixed", x, a, ib, fu, fd, 2, 2, fails)
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


@pytest.mark.parametrize("rs", aa_sets(), ids=lambda rs: "u{}d{}k{}k{}".format(*rs))
def test_general_kernel(dev, rs):
    ru, rd, ku, kd = rs
    fu, fd = aa_filters(ru, rd, ku, kd)
    fails = []
    for T in aa_lengths(ru, rd, kd):
        x, a, ib = aa_inputs(rs, T)
        rc, yg, ins = _run(dev, x, a, ib, fu, fd, ru, rd, False)
        what = f"general {rs} T {T} Tout {yg[1].shape[-1]}"
        if rc != 0:
            fails.append(f"{what}: return code {rc}")
            continue
        _check(what, yg, ins, rs, x, a, ib, fu, fd, ru, rd, fails)
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


def _golden_coeffs(alpha, beta):
    s = M.SnakeBeta(alpha.size, alpha_logscale=True)
    with torch.no_grad():
        s.alpha.copy_(torch.from_numpy(alpha))
        s.beta.copy_(torch.from_numpy(beta))
    return [t.contiguous() for t in s._host_coeffs()]


def test_goldens_through_the_raw_calls(dev, golden):
    """The recorded reference outputs (float32) at the goldens' own T, to the existing 2e-6: the general kernel on the
    six ratio sets, the fixed kernel on aa_activation.npz: the restatement and the recordings judge the same kernels."""
    gd = golden("aa_activation_ratios.npz")
    for ci, (ru, rd, ku, kd) in enumerate(aa_golden_sets()):
        fu, fd = aa_filters(ru, rd, ku, kd)
        for T in gd["meta"]["T"]:
            k = f"c{ci}_T{T}"
            x = torch.from_numpy(gd[f"x_{k}"])
            a, ib = _golden_coeffs(gd[f"alpha_{k}"], gd[f"beta_{k}"])
            rc, yg, ins = _run(dev, x, a, ib, fu, fd, ru, rd, False)
            want = torch.from_numpy(gd[f"y_{k}"])
            assert rc == 0 and tuple(yg[1].shape) == tuple(want.shape), (k, rc)
            assert _guards_intact(yg)
            assert_close_rel(yg[1].cpu(), want, 2e-6, f"aa ratios {(ru, rd, ku, kd)} T={T}")
    gd = golden("aa_activation.npz")
    fu, fd = torch.from_numpy(gd["up_filter"]).reshape(-1), torch.from_numpy(gd["down_filter"]).reshape(-1)
    assert torch.equal(fu, aa_filters(2, 2, 12, 12)[0]) and torch.equal(fd, aa_filters(2, 2, 12, 12)[1])
    for T in (1, 5, 37, 600):
        x = torch.from_numpy(gd[f"x_{T}"])
        a, ib = _golden_coeffs(gd[f"alpha_{T}"], gd[f"beta_{T}"])
        for fixed_entry in (True, False):
            rc, yg, ins = _run(dev, x, a, ib, fu, fd, 2, 2, fixed_entry)
            assert rc == 0 and _guards_intact(yg)
            assert_close_rel(yg[1].cpu(), torch.from_numpy(gd[f"y_{T}"]), 2e-6, f"aa T={T}")


@pytest.mark.parametrize("rs", AA_REFUSED, ids=lambda rs: "u{}d{}k{}k{}".format(*rs))
def test_refused(dev, rs):
    """More than 256 taps, a ratio above 16, fewer up taps than the up ratio: BC_ERR_UNSUPPORTED, nothing written."""
    ru, rd, ku, kd = rs
    x, a, ib = aa_inputs(rs, 37)
    rc, yg, ins = _run(dev, x, a, ib, torch.ones(ku) / ku, torch.ones(kd) / kd, ru, rd, False)
    assert rc == 3, rc
    assert _untouched(yg) and all(_guards_intact(g) for g in ins)


def test_zz_worst_ratio():
    """Runs last: the module's largest err / own (recorded in DESIGN.md; the bound allows 4)."""
    print(f"anti-aliased Snake: worst err / own {WORST[0]:.2f} at {WORST[1]}")
    assert WORST[1], "no case ran"
