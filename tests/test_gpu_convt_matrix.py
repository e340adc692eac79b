"""ConvTranspose1d (bc_convT1d_fwd, bc_convT1d_fwd_ws, convT_interleave_kernel) against float64 on the MI355X.

One item per (precision family fp32 / x6 / bf16 / h3, geometry of tests/test_convt_matrix_host.py).  An item loops over
the table's widths and input lengths and, per case, runs the raw C calls -- the strided-store path and the workspace
path with a workspace of exactly bc_convT1d_workspace_floats floats (none at stride 17, beyond the interleave's table)
-- with bias, without, with the Snake alone and with the dual raw + Snake output.  The weights are packed per phase for
the tile the library chooses (ConvTranspose1dWN.phase_cfg(B, Tin): lengths <= 128 take the narrow-launch tile); x, y,
y2 and the workspace sit between NaN guard bands and the outputs start as NaN.  Checked per case:
  - y against float64 F.conv_transpose1d on the weight-normed weight (tests/convt_ref.py) within the suite's conv
    tolerance(family, Cin, Kp); the Snake outputs against the float64 Snake of that reference with the conv matrix's
    widening (x 4 for the fp32-class families, x 1 for bf16);
  - no NaN left in an output, no band touched, on either path;
  - the dual run's raw output bit-identical to the run without Snake;
  - the workspace path bit-identical to the strided-store path, every epilogue.
On lengths 4, 5 and 65 at width (44, 24): y (and y2) 4 bytes off 16-byte alignment -- the interleave's scalar branch at
Tout % 4 == 0 -- and the registered torch op (ConvTranspose1dWN.run / CausalConvTranspose1d.run), both bit-identical to
the raw call; a case that failed a check between the bands is not handed to the op, whose own workspace has none.
At Tin = 64 the narrow-launch tile against the default tile: bit-identical in x6 and bf16 ("same K order
per output", x6_narrow_cfg), within the tolerance in h3.  Every failure of an item is collected before it asserts.

The module's last test lists the kernel instantiations the launches reached."""
import pytest
import torch

import convt_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import conv as CV
from test_conv_matrix_host import B, clip_rel_err, launched_name, tolerance
from test_convt_matrix_host import (GEOMS, ITEMS, MAX_WS_STRIDE, REFUSED, SUBSET_T, SUBSET_W, TILE_T, case_data,
                                    default_cfg, geom_id, item_cases, launch_cfg)
from test_gpu_conv_matrix import _guarded, _guards_intact, _sync, _untouched

pytestmark = pytest.mark.gpu

LAUNCHED = set()   # (family, kernel instantiation, taps per phase, output stride of the direct path's store)
TILE_PAIRS = {}    # family -> number of (narrow tile, default tile) comparisons made
WORST = {}         # family -> [worst y err / tol, worst Snake err / tol]
EPIS = ("bias", "nobias", "snake", "dual")


def _st():
    return torch.cuda.current_stream().cuda_stream


class _Outs:
    """NaN-initialised guarded y (and y2), off floats past 16-byte alignment."""

    def __init__(self, dev, cd, dual, off=0):
        self.y = _guarded(dev, (B, cd.Cout, cd.Tout), off)
        self.y2 = _guarded(dev, (B, cd.Cout, cd.Tout), off) if dual else None

    def ptrs(self):
        return self.y[1].data_ptr(), self.y2[1].data_ptr() if self.y2 else None

    def tensors(self):
        return [("y", self.y)] + ([("y2", self.y2)] if self.y2 else [])


def _call(cd, xg, prep, cfg, epi, outs, ws=None, Bn=B, Tout=None):
    """One raw call: bc_convT1d_fwd, or bc_convT1d_fwd_ws when ws is a guarded workspace."""
    lib = L.load()
    g = cd.g
    _, wptrs, bias, _ = prep
    sa, sb = cd.coeffs if epi in ("snake", "dual") else (None, None)
    y, y2 = outs.ptrs()
    args = (xg[1].data_ptr(), wptrs, L.ptr(bias) if epi != "nobias" else None, L.ptr(sa), L.ptr(sb), y, y2, Bn, cd.Cin,
            cd.Tin, cd.Cout, cd.Tout if Tout is None else Tout, g.K, g.s, g.p, cfg)
    if ws is None:
        return lib.bc_convT1d_fwd(*args, _st())
    return lib.bc_convT1d_fwd_ws(*args, ws[1].data_ptr(), _st())


def _workspace(dev, cd, dual):
    """A guarded workspace of exactly the floats the library asks for (None beyond the interleave's table)."""
    g = cd.g
    n = L.load().bc_convT1d_workspace_floats(B, cd.Cout, cd.Tout, g.K, g.s, g.p, int(dual))
    assert (n < 0) == (g.s > MAX_WS_STRIDE)
    # s * B * Cout * Q4 with Q4 a multiple of 4: the phase rows stay 16-byte aligned (the 16-byte epilogue)
    assert n < 0 or n == R.workspace_floats(B, cd.Cout, cd.Tout, g.s, g.p, dual), (geom_id(g), cd.Cout, cd.Tout, n)
    return _guarded(dev, (n,)) if n > 0 else None


def _note_launch(family, cfg, cd):
    name = launched_name(cfg, cd.Kp, 1, 1, cd.Tin, 0)
    LAUNCHED.add((family, name, cd.Kp, cd.g.s))
    return name


def _bits_equal(a, b):
    return torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _run_case(dev, family, cd, fails):
    """The four epilogues of one case on both paths; appends a line per failed check."""
    g = cd.g
    cfg = launch_cfg(family, cd.Cin, cd.Cout, cd.Kp, cd.Tin)
    fam = "fp32" if cfg < 100 else family
    tol = tolerance(fam, cd.Cin, cd.Kp)
    tol2 = tol * (4 if fam != "bf16" else 1)
    prep = cd.m.prepared(dev, cfg)
    cd.coeffs = cd.snake.coeffs(dev)
    xg = _guarded(dev, (B, cd.Cin, cd.Tin), 0, cd.x)
    name = _note_launch(family, cfg, cd)
    what0 = f"{family} {geom_id(g)} {cd.Cin}->{cd.Cout} Tin {cd.Tin} Tout {cd.Tout} cfg {cfg}"
    raw_bias = None
    errs = [0.0, 0.0]
    for epi in EPIS:
        what = f"{what0} {epi}"
        dual = epi == "dual"
        direct, viaws = _Outs(dev, cd, dual), _Outs(dev, cd, dual)
        try:
            wsg = _workspace(dev, cd, dual)
        except AssertionError as e:
            fails.append(f"{what}: bc_convT1d_workspace_floats is not the restated s * B * Cout * Q4: {e}")
            continue
        rc = _call(cd, xg, prep, cfg, epi, direct)
        rc_ws = _call(cd, xg, prep, cfg, epi, viaws, ws=wsg) if wsg is not None else 0
        _sync(what)
        if rc != 0 or rc_ws != 0:
            fails.append(f"{what}: return codes {rc} (direct) {rc_ws} (workspace)")
            continue
        if not _guards_intact(xg) or (wsg is not None and not _guards_intact(wsg)):
            fails.append(f"{what}: the band of x or of the workspace was written")
        want, want_act = cd.want(epi != "nobias")
        for path, o in (("direct", direct),) + ((("workspace", viaws),) if wsg is not None else ()):
            for nm, t in o.tensors():
                if not _guards_intact(t):
                    fails.append(f"{what} {path}: {nm} written outside the tensor")
                got = t[1].cpu()
                n_nan = int((~torch.isfinite(got)).sum())
                if n_nan:
                    fails.append(f"{what} {path}: {nm} has {n_nan} non-finite elements of {got.numel()}")
                    continue
                if path == "workspace":
                    continue  # compared bitwise with the direct path below
                act = nm == "y2" or epi == "snake"
                w, tl = (want_act, tol2) if act else (want, tol)
                err = clip_rel_err(got, w)
                errs[act] = max(errs[act], err / tl)
                if err > tl:
                    fails.append(f"{what}: {nm} rel err {err:.3e} > {tl:.1e}{_where(got, w, g)}")
        if wsg is not None:
            for (nm, a), (_, b) in zip(direct.tensors(), viaws.tensors()):
                if not _bits_equal(a, b):
                    fails.append(f"{what}: {nm} of the workspace path differs from the direct path"
                                 f"{_where(b[1].cpu(), a[1].cpu().double(), g)}")
        if epi == "bias":
            raw_bias = direct.y
        elif dual and not _bits_equal(direct.y, raw_bias):
            fails.append(f"{what}: the raw output differs from the run without Snake")
    w = WORST.setdefault(fam, [0.0, 0.0])
    w[0], w[1] = max(w[0], errs[0]), max(w[1], errs[1])
    print(f"{what0}: y err {errs[0] * tol:.3e} (bound {tol:.1e}), Snake err {errs[1] * tol2:.3e} (bound {tol2:.1e}), "
          f"{name}")
    return xg, prep, cfg, raw_bias


def _where(got, want, g):
    """' at t = ... (phase r, q = ...)' of the largest difference (NaN counts as largest)."""
    d = (got.double() - want).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    t = int(d.flatten(0, 1).max(0)[0].argmax())
    return f"; worst at t = {t} (phase {(t + g.p) % g.s}, q = {(t + g.p) // g.s})"


def _run_subset(dev, family, cd, xg, prep, cfg, fails):
    """Misaligned outputs on the workspace path, and the registered op, against the aligned direct call."""
    g = cd.g
    what0 = f"{family} {geom_id(g)} {cd.Cin}->{cd.Cout} Tin {cd.Tin} cfg {cfg}"
    n_fails = len(fails)
    base = {}
    for epi in ("bias", "dual"):
        base[epi] = _Outs(dev, cd, epi == "dual")
        L.check(_call(cd, xg, prep, cfg, epi, base[epi]), "bc_convT1d_fwd")
    _sync(what0)
    if cd.Tout % 4 == 0 and g.s <= MAX_WS_STRIDE:
        for epi in ("bias", "dual"):
            off1 = _Outs(dev, cd, epi == "dual", off=1)
            wsg = _workspace(dev, cd, epi == "dual")
            rc = _call(cd, xg, prep, cfg, epi, off1, ws=wsg)
            _sync(f"{what0} {epi} y 4 bytes off")
            for (nm, a), (_, b) in zip(base[epi].tensors(), off1.tensors()):
                if rc != 0 or not _guards_intact(b) or not _bits_equal(a, b):
                    fails.append(f"{what0} {epi}: {nm} 4 bytes off alignment: rc {rc}, bands intact "
                                 f"{_guards_intact(b)}{_where(b[1].cpu(), a[1].cpu().double(), g)}")
    if len(fails) > n_fails:
        return
    # the registered op (which sizes its own workspace, none at stride 17)
    if g.crop == g.s and g.p == 0 and g.opad == 0:
        m = CV.CausalConvTranspose1d(cd.Cin, cd.Cout, g.K, g.s)
        m.conv.load_state_dict(cd.m.state_dict())
    else:
        m = CV.ConvTranspose1dWN(cd.Cin, cd.Cout, g.K, g.s, padding=g.p, output_padding=g.opad)
        m.load_state_dict(cd.m.state_dict())
        m.causal_crop = g.crop
    m.to(dev)
    y = m.run(xg[1])
    raw, act = m.run(xg[1], out_snake=cd.coeffs, dual=True)
    _sync(f"{what0} op")
    for nm, got, want in (("y", y, base["bias"].y), ("raw", raw, base["dual"].y), ("act", act, base["dual"].y2)):
        w = want[1]
        if tuple(got.shape) != tuple(w.shape) or not torch.equal(got.view(torch.int32), w.view(torch.int32)):
            fails.append(f"{what0}: the op's {nm} differs from the raw call")


def _run_tile_pair(dev, family, cd, fails):
    """At Tin = 64: the narrow-launch tile against the default tile (both through the direct path)."""
    narrow, wide = launch_cfg(family, cd.Cin, cd.Cout, cd.Kp, cd.Tin), default_cfg(family, cd.Cin, cd.Cout, cd.Kp)
    if narrow == wide:
        return
    xg = _guarded(dev, (B, cd.Cin, cd.Tin), 0, cd.x)
    tol = tolerance(family, cd.Cin, cd.Kp)
    name = _note_launch(family, wide, cd)
    what0 = f"{family} {geom_id(cd.g)} {cd.Cin}->{cd.Cout} Tin {cd.Tin} tiles {narrow} / {wide}"
    for epi in ("bias", "dual"):
        outs = {}
        for cfg in (narrow, wide):
            outs[cfg] = _Outs(dev, cd, epi == "dual")
            L.check(_call(cd, xg, cd.m.prepared(dev, cfg), cfg, epi, outs[cfg]), "bc_convT1d_fwd")
        _sync(f"{what0} {epi}")
        want = cd.want(True)
        for i, ((nm, a), (_, b)) in enumerate(zip(outs[narrow].tensors(), outs[wide].tensors())):
            tl = tol * (4 if i and family != "bf16" else 1)
            err = clip_rel_err(b[1].cpu(), want[i])
            if not _guards_intact(b) or not err <= tl:
                fails.append(f"{what0} {epi}: {nm} of the default tile: rel err {err:.3e} > {tl:.1e} or a band written")
            if family in ("x6", "bf16") and not _bits_equal(a, b):
                fails.append(f"{what0} {epi}: {nm} depends on the tile"
                             f"{_where(a[1].cpu(), b[1].cpu().double(), cd.g)}")
    TILE_PAIRS[family] = TILE_PAIRS.get(family, 0) + 1
    print(f"{what0}: compared, default tile {name}")


@pytest.mark.parametrize("family,g", ITEMS, ids=[f"{f}-{geom_id(g)}" for f, g in ITEMS])
def test_convt(dev, family, g):
    old = L.precision_mode()
    L.set_precision(family)
    fails, n = [], 0
    try:
        for Cin, Cout, Tin in item_cases(family, g):
            cd = case_data(g, Cin, Cout, Tin)
            n_fails = len(fails)
            xg, prep, cfg, _ = _run_case(dev, family, cd, fails)
            # (the op allocates its own workspace, without bands: only a case that is right between bands goes on to it)
            if (Cin, Cout) == SUBSET_W and Tin in SUBSET_T and len(fails) == n_fails:
                _run_subset(dev, family, cd, xg, prep, cfg, fails)
            if Tin == TILE_T and family != "fp32":
                _run_tile_pair(dev, family, cd, fails)
            n += 1
    finally:
        L._mode = old
    assert n >= 24
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


@pytest.mark.parametrize("family", ["fp32", "x6"])
def test_refused_and_empty(dev, family):
    """padding > s (Kp - 1) -- (2, 4, 3) and (4, 4, 1), both with padding < K -- returns BC_ERR_UNSUPPORTED from both
    entry points; B = 0 and Tout = 0 return BC_OK; none of them writes an output or the workspace."""
    old = L.precision_mode()
    L.set_precision(family)
    try:
        for g in REFUSED + [GEOMS[0]]:
            cd = case_data(g, 44, 24, 5)
            assert R.supported(g.s, g.K, g.p) == (g not in REFUSED) and cd.Tout > 0
            cfg = launch_cfg(family, cd.Cin, cd.Cout, cd.Kp, cd.Tin)
            prep = cd.m.prepared(dev, cfg)
            cd.coeffs = cd.snake.coeffs(dev)
            xg = _guarded(dev, (B, cd.Cin, cd.Tin), 0, cd.x)
            kinds = [dict()] if g in REFUSED else [dict(Bn=0), dict(Tout=0)]
            for kw in kinds:
                for epi in ("bias", "dual"):
                    for use_ws in (False, True):
                        outs = _Outs(dev, cd, epi == "dual")
                        wsg = _workspace(dev, cd, epi == "dual") if use_ws else None
                        rc = _call(cd, xg, prep, cfg, epi, outs, ws=wsg, **kw)
                        _sync(f"{family} {geom_id(g)} {kw} {epi}")
                        assert rc == (3 if g in REFUSED else 0), (g, kw, epi, use_ws, rc)
                        assert all(_untouched(t) for _, t in outs.tensors()), (g, kw, epi, use_ws)
                        assert wsg is None or _untouched(wsg), (g, kw, epi)
    finally:
        L._mode = old


def _variant(name):
    """(pointwise, 16-byte input staging) of a kernel instantiation's name."""
    if name.startswith("conv1d_x6ra_kernel"):
        return False, name.endswith("<true>")
    a = name[name.index("<") + 1:-1].split(", ")
    return a[5] == "true", a[8] == "true"


def test_zz_launches_reached_the_variants():
    """Runs last: lists the instantiations the launches above reached and asserts, per x6-family precision, a pointwise
    variant storing at an output stride > 1, a multi-tap variant with 16-byte input staging and one without, and that
    narrow-launch and default tiles were compared; the fp32 kernel (one variant per tile) ran one-tap and multi-tap
    phases at an output stride > 1."""
    for fam in ("fp32", "x6", "bf16", "h3"):
        rows = sorted((n, kp, s) for f, n, kp, s in LAUNCHED if f == fam)
        names = sorted({n for n, _, _ in rows})
        print(f"{fam}: {len(names)} instantiations, worst y err / tol {WORST.get(fam, [0, 0])[0]:.3f}, "
              f"worst Snake err / tol {WORST.get(fam, [0, 0])[1]:.3f}, {TILE_PAIRS.get(fam, 0)} tile pairs")
        for n in names:
            print(f"  {n}: (taps, stride) {sorted({(kp, s) for m, kp, s in rows if m == n})}")
        if fam == "fp32":
            assert all(n.startswith("conv1d_mfma_kernel") for n in names)
            assert any(kp == 1 and s > 1 for _, kp, s in rows) and any(kp > 1 and s > 1 for _, kp, s in rows)
            continue
        assert all(n.startswith("conv1d_x6") for n in names), names
        var = [(_variant(n), kp, s) for n, kp, s in rows]
        assert any(pw and s > 1 for (pw, _), kp, s in var), f"{fam}: no pointwise variant at an output stride > 1"
        assert any(not pw and b4 and kp > 1 for (pw, b4), kp, s in var), f"{fam}: no multi-tap 16-byte staging"
        assert any(not pw and not b4 and kp > 1 for (pw, b4), kp, s in var), f"{fam}: no multi-tap variant without it"
        assert TILE_PAIRS.get(fam, 0) >= len(GEOMS), (fam, TILE_PAIRS)
