"""Every one-launch ResidualUnit kernel instantiation against fp64 on the MI355X.

test_resunit_item: one item per kernel name of the host enumeration (tests/resunit_ref.py items(): 32
resunit_x6_kernel instantiations, the 16-wave unit at C = 192 in x6 and bf16, the three strip kernels and resunit_rr at
C = 48 in h3), calling bc_resunit_fwd / bc_resunit_fwd_snake_in directly with weights packed for the item's cfg.  Per
dilation (1, 3, 9; 2, 5, 8 on resunit_rr; a strip kernel's own) and per tile width BN of the item's family and width:
T = BN + 40 with every tensor aligned (layout A) and with y / y2 4 bytes off (M: scalar epilogue under 16-byte
staging), T = BN + 37 with causal padding and x_raw / x_act 4 bytes off (U), and T = 5 (below the halo at d = 3 and 9)
with both paddings.  Each in four input / output modes: a producer-side x_act, snake on load, snake on load with the
dual output y + y2, and snake on load with the activated output only.  x_raw, x_act, y and y2 sit between NaN guard
bands.  Checked: return code, guard bands bit-intact, finite output, the error against the fp64 definition within
resunit_ref.bound (bf16: the suite's bf16 criteria), the four modes bitwise equal, the 16-wave x6 unit within 2e-6 of
the two-launch path, and the refusals (d = 10, a tile of another width, cfg 322) that must leave y untouched.  Every
failed check of an item is collected before it asserts.

test_zy_cfgs_bit_identical: per (family, C, d, padding, T, layout) the outputs of all cfgs of the family and width,
compared bitwise.  test_zz_launch_set_covers_the_host_list: every item ran in every mode and layout.

The strip kernels run with one block per strip at these sizes (2 clips x at most 5 blocks on 256 CUs: B * blocks / CUs
< 1); test_gpu_kernels' test_strip_partition_independent ties longer strips to that partition bit for bit."""
import functools
import hashlib
import time

import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import blocks as BL
from audiotokenization_amd import modules as M
from audiotokenization_amd.blocks import _conv_of, produce_conv
from helpers import max_rel_err
from resunit_ref import (B, IO_MODES, LAYOUTS, bound, clip_err, cpu32, data, item_cases, item_id, items, ref64, worst)

pytestmark = pytest.mark.gpu

GUARD = 256
NAN_BITS = 0x7FC00000
BC_ERR_ARG = 1
LAUNCHED = set()   # (kernel name, input / output mode, layout)
DIGESTS = {}       # (family, C, d, causal, T, layout) -> {cfg: (BN, digest of y and y2)}
RATIOS = {}        # item id -> {"raw" / "act": largest (kernel error) / cpu32}
TIMES = {}         # item id -> seconds


def _sync(what):
    """Wait for the launch; a device fault ends the whole run (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after {what}: {e}", returncode=3)


def _guarded(dev, shape, off=0, src=None):
    """A tensor of `shape` inside a NaN-filled buffer, GUARD floats of it on each side; the tensor starts `off` floats
    past a 16-byte aligned address."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + off + n + GUARD,), float("nan"), device=dev)
    view = buf[GUARD + off:GUARD + off + n].view(shape)
    assert view.data_ptr() % 16 == 4 * (off % 4)
    if src is not None:
        view.copy_(src)
    return buf, view, off


def _guards_intact(g):
    buf, view, off = g
    bits = buf.view(torch.int32)
    lo, hi = GUARD + off, GUARD + off + view.numel()
    return bool((bits[:lo] == NAN_BITS).all()) and bool((bits[hi:] == NAN_BITS).all())


def _untouched(g):
    return bool((g[0].view(torch.int32) == NAN_BITS).all())


@functools.lru_cache(maxsize=None)
def _unit(case):
    """The package's ResidualUnit with the case's parameters (on the host: its convs pack per cfg and cache that) and
    the next Snake."""
    ru = BL.ResidualUnit(case.C, dilation=case.d, causal=case.causal)
    p = data(case)
    ru.load_state_dict(p.sd, strict=True)
    nxt = M.Activation1d(activation=M.SnakeBeta(case.C, alpha_logscale=True))
    with torch.no_grad():
        nxt.act.alpha.copy_(p.next_alpha)
        nxt.act.beta.copy_(p.next_beta)
    return ru.eval(), nxt.eval()


@functools.lru_cache(maxsize=None)
def _two_launch(family, case, dev):
    """The unit as two bc_conv1d_fwd launches in the family's precision (k = 7 conv writing snake(h), k = 1 conv adding
    the skip), on aligned tensors."""
    ru, _ = _unit(case)
    old = L.precision_mode()
    L.set_precision(family)
    try:
        ru.to(dev)
        xd = data(case).x.to(dev)
        xa = ru.first_act(xd)
        _, h = produce_conv(ru.block[1], xa, None, want_raw=False, next_act=ru.block[2])
        two = produce_conv(ru.block[3], h, residual=xd, want_raw=True, next_act=None)[0]
        _sync(f"two launches {family} {case}")
        return two.cpu()
    finally:
        L._mode = old


def _launch(lib, st, mode, a):
    """One launch in input / output mode `mode`; returns (return code, guarded y, guarded y2 or None)."""
    dual, act_only = mode == "sin_dual", mode == "sin_act"
    yg = _guarded(a.dev, a.shape, a.yoff)
    y2g = _guarded(a.dev, a.shape, a.yoff) if dual else None
    osa, osb = (a.osa, a.osb) if dual or act_only else (None, None)
    tail = (a.w7.data_ptr(), L.ptr(a.b7), a.s2a.data_ptr(), a.s2b.data_ptr(), a.w1.data_ptr(), L.ptr(a.b1), L.ptr(osa),
            L.ptr(osb), yg[1].data_ptr(), y2g[1].data_ptr() if dual else None, B, a.C, a.T, a.d, a.pl, a.cfg, st)
    if mode == "xact":
        rc = lib.bc_resunit_fwd(a.xg[1].data_ptr(), a.xag[1].data_ptr(), *tail)
    else:
        rc = lib.bc_resunit_fwd_snake_in(a.xg[1].data_ptr(), a.s1a.data_ptr(), a.s1b.data_ptr(), *tail)
    _sync(f"{a.what} {mode}")
    return rc, yg, y2g


class _Args:
    pass


def _run_case(dev, it, case, layout, fails, ratios):
    """All four input / output modes of one case in one layout; appends a line per failed check."""
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    ru, nxt = _unit(case)
    ru.to(dev)
    nxt.to(dev)
    conv7, conv1 = _conv_of(ru.block[1]), _conv_of(ru.block[3])
    p = data(case)
    a = _Args()
    a.dev, a.C, a.T, a.d, a.cfg, a.pl = dev, case.C, case.T, case.d, it.cfg, conv7.pad_left()
    assert a.pl == (6 if case.causal else 3) * case.d
    a.shape = (B, case.C, case.T)
    a.w7, a.b7 = conv7.packed_as(it.cfg, dev)
    a.w1, a.b1 = conv1.packed_as(it.cfg, dev)
    a.s1a, a.s1b = ru.block[0].act.coeffs(dev)
    a.s2a, a.s2b = ru.block[2].act.coeffs(dev)
    a.osa, a.osb = nxt.act.coeffs(dev)
    xoff = 1 if layout == "U" else 0
    a.yoff = 1 if layout == "M" else 0
    assert layout == "U" or case.T % 4 == 0 or case.T == 5
    xd = p.x.to(dev)
    a.xg = _guarded(dev, a.shape, xoff, xd)
    a.xag = _guarded(dev, a.shape, xoff, ru.first_act(xd))
    a.what = f"cfg {it.cfg} C {case.C} d {case.d} {'causal' if case.causal else 'centred'} T {case.T} layout {layout}"
    name = L.resunit_kernel_name(it.cfg, case.C, case.d)
    if name != it.name:
        fails.append(f"{a.what}: launches {name}, not the item's {it.name}")
    want, want_act = ref64(case)
    c32 = cpu32(case)
    outs = {}
    for mode in IO_MODES:
        rc, yg, y2g = _launch(lib, st, mode, a)
        what = f"{a.what} {mode}"
        if rc != 0:
            fails.append(f"{what}: return code {rc}")
            continue
        LAUNCHED.add((name, mode, layout))
        for nm, g in (("y", yg), ("y2", y2g), ("x_raw", a.xg), ("x_act", a.xag)):
            if g is not None and not _guards_intact(g):
                fails.append(f"{what}: written outside {nm}")
        if not torch.equal(a.xg[1], xd):
            fails.append(f"{what}: x_raw was written")
        res = {"act" if mode == "sin_act" else "raw": yg[1].cpu()}
        if y2g is not None:
            res["act"] = y2g[1].cpu()
        outs[mode] = res
        for o, got in res.items():
            w = want if o == "raw" else want_act
            if not bool(torch.isfinite(got).all()):
                fails.append(f"{what}: {o} has {int((~torch.isfinite(got)).sum())} non-finite elements")
                continue
            err = clip_err(got, w)
            if it.family == "bf16":
                if err >= 2e-2:
                    fails.append(f"{what}: {o} rel err {err:.3e} >= 2e-2; {worst(got, w)}")
                if o == "raw" and err <= 1e-5:
                    fails.append(f"{what}: rel err {err:.3e}: not bf16 products")
                continue
            ratios[o] = max(ratios.get(o, 0.0), err / c32[o])
            bnd = bound(case, it.family, o)
            if err > bnd:
                fails.append(f"{what}: {o} rel err {err:.3e} > bound {bnd:.3e} ({err / c32[o]:.2f} x cpu32); "
                             f"{worst(got, w)}")
    # the four modes compute the same operations in the same order: equal bits
    raws = [(m, outs[m]["raw"]) for m in ("xact", "sin", "sin_dual") if m in outs]
    for m, t in raws[1:]:
        if not torch.equal(t, raws[0][1]):
            fails.append(f"{a.what}: y of mode {m} differs from mode {raws[0][0]}'s, max |d| "
                         f"{float((t - raws[0][1]).abs().max()):.3e}")
    if "sin_dual" in outs and "sin_act" in outs and not torch.equal(outs["sin_dual"]["act"], outs["sin_act"]["act"]):
        fails.append(f"{a.what}: the activated-only output differs from the dual output's y2")
    if "sin_dual" in outs:
        d = outs["sin_dual"]
        dig = hashlib.sha1(d["raw"].numpy().tobytes() + d["act"].numpy().tobytes()).hexdigest()
        DIGESTS.setdefault((it.family, case.C, case.d, case.causal, case.T, layout), {})[it.cfg] = (it.BN, dig)
    if raws and (it.family == "bf16" or it.C == 192):
        two = _two_launch(it.family, case, dev)
        tol = 1e-5 if it.family == "bf16" else 2e-6
        err = max_rel_err(raws[0][1], two)
        if err > tol:
            fails.append(f"{a.what}: one launch vs two: max |a-b| / max |b| = {err:.3e} > {tol:.0e}")


def _refusals(dev, it, fails):
    """d = 10, a tile of another width and cfg 322 return BC_ERR_ARG and leave y as it was."""
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    case, layout = item_cases(it)[0]
    ru, nxt = _unit(case)
    ru.to(dev)
    conv7, conv1 = _conv_of(ru.block[1]), _conv_of(ru.block[3])
    other = 100 * (it.cfg // 100) + (9 if it.C == 48 else 11)  # the 96-row tile at C = 48, else the 48-row tile
    for what, cfg, d in (("d = 10", it.cfg, 10), (f"cfg {other} (another width)", other, case.d), ("cfg 322", 322, case.d)):
        if lib.bc_resunit_kernel_name(cfg, case.C, d, None, 0) >= 0:
            fails.append(f"refusal {what} at C {case.C}: bc_resunit_kernel_name accepts it (not launched)")
            continue
        a = _Args()
        a.dev, a.C, a.T, a.d, a.cfg, a.pl = dev, case.C, case.T, d, cfg, 3 * d
        a.shape, a.yoff = (B, case.C, case.T), 0
        a.w7, a.b7 = conv7.packed_as(it.cfg, dev)
        a.w1, a.b1 = conv1.packed_as(it.cfg, dev)
        a.s1a, a.s1b = ru.block[0].act.coeffs(dev)
        a.s2a, a.s2b = ru.block[2].act.coeffs(dev)
        a.osa = a.osb = None
        a.xg = a.xag = _guarded(dev, a.shape, 0, data(case).x.to(dev))
        a.what = f"refusal {what} at C {case.C}"
        for mode in ("xact", "sin"):
            rc, yg, _ = _launch(lib, st, mode, a)
            if rc != BC_ERR_ARG:
                fails.append(f"{a.what} {mode}: return code {rc}, expected BC_ERR_ARG")
            if not _untouched(yg):
                fails.append(f"{a.what} {mode}: y was written")


ITEMS = items()


@pytest.mark.parametrize("it", ITEMS, ids=[item_id(i) for i in ITEMS])
def test_resunit_item(dev, it):
    t0 = time.perf_counter()
    fails, ratios = [], {}
    n = 0
    for case, layout in item_cases(it):
        _run_case(dev, it, case, layout, fails, ratios)
        n += 1
    _refusals(dev, it, fails)
    assert n >= 5 * len(it.dils) and len(it.dils) >= 1
    TIMES[item_id(it)] = time.perf_counter() - t0
    RATIOS[item_id(it)] = ratios
    print(f"{item_id(it)} ({it.name}): {n} cases x {len(IO_MODES)} modes in {TIMES[item_id(it)]:.2f} s; "
          f"largest error / cpu32: " + (", ".join(f"{o} {v:.2f}" for o, v in sorted(ratios.items(), reverse=True))
                                        or "(bf16 criteria)"))
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


def test_zy_cfgs_bit_identical():
    """Per (family, C, d, padding, T, layout): the y and y2 of every cfg of the family and width, compared bitwise.
    Every tile walks K in the same order per output, so each group must be one class.  Measured on the MI355X: it is, in
    all 441 groups -- in h3 too, where tiles of different column counts take their block scales (powers of two) from
    different sets of columns: 305 / 310 at C = 64 and 304 / 309 / 316 / 323 at C = 96 give the same bits on these
    data."""
    assert DIGESTS, "test_resunit_item did not run"
    bad = []
    summary = {}
    for key, by_cfg in sorted(DIGESTS.items()):
        family = key[0]
        groups = {}
        for cfg, (bn, dig) in sorted(by_cfg.items()):
            groups.setdefault(dig, []).append(cfg)
        classes = sorted(groups.values())
        summary.setdefault((family, key[1], tuple(map(tuple, classes))), []).append(key[2:])
        want_cfgs = {it.cfg for it in ITEMS if (it.family, it.C) == key[:2] and key[2] in it.dils}
        if set(by_cfg) != want_cfgs:
            bad.append(f"{key}: cfgs {sorted(by_cfg)} ran, the family and width have {sorted(want_cfgs)}")
        if len(classes) > 1:
            bad.append(f"{key}: bit-identity classes {classes}")
    for (family, C, classes), keys in sorted(summary.items()):
        print(f"{family} C {C}: bit-identity classes {[list(c) for c in classes]} in {len(keys)} groups"
              + ("" if len(classes) == 1 else f" (d, causal, T, layout) {keys}"))
    assert not bad, f"{len(bad)} groups split:\n" + "\n".join(bad)


def test_zz_launch_set_covers_the_host_list():
    """Runs last: every item of the host list was launched in every input / output mode and layout (so an instantiation
    cannot drop out of the matrix unnoticed).  Prints the slowest item and the items' total."""
    want = {(it.name, m, lay) for it in ITEMS for m in IO_MODES for lay in LAYOUTS}
    print(f"launched {len({n for n, _, _ in LAUNCHED})} distinct unit instantiations, the host list has {len(ITEMS)}")
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"slowest item {slow}: {TIMES[slow]:.2f} s; all items {sum(TIMES.values()):.1f} s")
    for fam in ("x6", "h3"):
        for o in ("raw", "act"):
            r = {k: v[o] for k, v in RATIOS.items() if k.startswith(fam) and o in v}
            if r:
                k = max(r, key=r.get)
                print(f"largest {fam} {o} error / cpu32: {r[k]:.3f} ({k})")
    assert not want - LAUNCHED, sorted(want - LAUNCHED)
