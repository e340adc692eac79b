"""Every conv tile, precision and kernel variant against fp64 on the MI355X.

Part 1 (test_conv_tile): one item per (precision family, tile) -- the 23 x6-family tiles as x6 / bf16 / h3 and the 20
fp32 MFMA cfgs -- calling bc_conv1d_fwd directly over the shape classes of tests/test_conv_matrix_host.py (pointwise,
k7, k7 d9, k3, k2, direct and phase-decomposed stride 2 / 4 / 5, a one-tap phase conv, a causal k7 d9), at
Cout = BM + 8 / BM - 11 / 1, two clips scaled 1x and 37x (1/37x on k7, see CLIP_SCALE_TANH), Tout = BN + 40 (aligned:
16-byte epilogue and staging) and BN + 37 (input 4 bytes off: scalar epilogue, single-float staging, ragged last column
tile), with bias, without, with residual + Snake dual output, and tanh.  The reference is fp64 F.conv1d on the
weight-normed weight plus the epilogue in fp64; x, y, y2 and the residual sit between NaN guard bands;
BC_ERR_UNSUPPORTED is allowed exactly where the documented limits say so and must leave the output untouched.  Every
failure of an item is collected before it asserts.

Part 2 (test_width_sweep, test_ngf40_model): widths no preset has, through the library's own tile choice.

Bit-identity (test_tiles_bit_identical): "same K order per output: x6 and bf16 results do not depend on the tile"
(x6_narrow_cfg).  Measured classes are recorded in DESIGN.md.

The module's last test checks that the launches covered every kernel instantiation the host enumeration lists."""
import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import conv as CV
from audiotokenization_amd import modules as M
from helpers import assert_close_rel, build_models, index_mismatches, top2_gap, torch_sd
from oracle import bigcodec_oracle as O
from test_conv_matrix_host import (B, BITID_COUT, BITID_TOUT, CIN, CLASSES, FAMILIES, GUARD, ITEMS, MODES, N_X6_TILES,
                                   WIDTHS, case_data, clip_rel_err, conv_pad, in_len, item_cases, launched_name,
                                   matrix_names, supported, sweep_shapes, tolerance)

pytestmark = pytest.mark.gpu

LAUNCHED = set()  # kernel instantiations launched by this module, checked by its last test
NAN_BITS = 0x7FC00000


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


def _snake_coeffs(cd, dev):
    s = M.SnakeBeta(cd.Cout, alpha_logscale=True)
    with torch.no_grad():
        s.alpha.copy_(cd.alpha)
        s.beta.copy_(cd.beta)
    return s.to(dev).coeffs(dev)


def _run_case(dev, family, c, fails):
    """All epilogues of one case; appends a line per failed check."""
    cls = c.cls
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    cd = case_data(cls, c.Cin, c.Cout, c.Tin)
    assert cd.Tout == c.Tout
    expect = supported(c.cfg, cls.K, cls.s, cls.d)
    wp, bias = cd.m.packed_as(c.cfg, dev)
    xg = _guarded(dev, (B, c.Cin, c.Tin), c.xoff, cd.x)
    tol = tolerance(family, c.Cin, cls.K)
    what0 = f"cfg {c.cfg} {cls.name} Cout {c.Cout} Tout {c.Tout} xoff {c.xoff}"
    for epi in (c.epis if expect else c.epis[:1]):
        what = f"{what0} {epi}"
        dual = epi == "res_snake"
        yg = _guarded(dev, (B, c.Cout, c.Tout))
        y2g = _guarded(dev, (B, c.Cout, c.Tout)) if dual else None
        rg = _guarded(dev, (B, c.Cout, c.Tout), 0, cd.res) if dual else None
        sa, sb = _snake_coeffs(cd, dev) if dual else (None, None)
        rc = lib.bc_conv1d_fwd(xg[1].data_ptr(), wp.data_ptr(), L.ptr(bias) if epi != "nobias" else None,
                               rg[1].data_ptr() if dual else None, L.ptr(sa), L.ptr(sb), yg[1].data_ptr(),
                               y2g[1].data_ptr() if dual else None, B, c.Cin, c.Tin, c.Cout, c.Tout, cls.K, cls.s, cls.d,
                               c.pad, int(epi == "tanh"), c.cfg, st)
        _sync(what)
        if rc == 3:
            if expect:
                fails.append(f"{what}: BC_ERR_UNSUPPORTED, but the documented limits admit it")
            if not _untouched(yg) or (dual and not _untouched(y2g)):
                fails.append(f"{what}: BC_ERR_UNSUPPORTED, but the output was written")
            continue
        if rc != 0:
            fails.append(f"{what}: return code {rc}")
            continue
        LAUNCHED.add(launched_name(c.cfg, cls.K, cls.s, cls.d, c.Tin, c.xoff))
        if not expect:
            fails.append(f"{what}: ran, but the documented limits say BC_ERR_UNSUPPORTED")
            continue
        want, want_act = cd.want(epi)
        for name, g, w, t in (("y", yg, want, tol), ("y2", y2g, want_act, tol * (4 if family != "bf16" else 1))):
            if g is None:
                continue
            if not _guards_intact(g):
                fails.append(f"{what}: {name} written outside the tensor")
            got = g[1].cpu()
            if not bool(torch.isfinite(got).all()):
                fails.append(f"{what}: {name} has {int((~torch.isfinite(got)).sum())} non-finite elements")
                continue
            err = clip_rel_err(got, w)
            if err > t:
                fails.append(f"{what}: {name} rel err {err:.3e} > {t:.1e}")
            if family == "bf16" and name == "y" and err <= 1e-5:
                fails.append(f"{what}: rel err {err:.3e}: not bf16 products")


@pytest.mark.parametrize("family,cfg0", ITEMS, ids=[f"{f}-{c}" for f, c in ITEMS])
def test_conv_tile(dev, family, cfg0):
    fails = []
    n = 0
    for c in item_cases(family, cfg0):
        _run_case(dev, family, c, fails)
        n += 1
    assert n >= 2 * len([k for k in CLASSES if family != "fp32" or not k.phase])
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


# tiles the narrow-launch rule swaps between (x6_narrow_cfg): a stream's chunk and the whole clip must give the same bits
NARROW_SET = (12, 14, 15, 16, 17, 20, 21, 22)


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.name)
@pytest.mark.parametrize("family", ["x6", "bf16"])
def test_tiles_bit_identical(dev, family, cls):
    """x6 and bf16 outputs of every tile that runs the class, at a common Cout = 200 and Tout = 296 / 293, compared
    bitwise (a direct strided conv and its phase-decomposed form walk K in different orders: each is its own class).
    Epilogues: bias, no bias, residual + Snake dual output, and tanh on the k7 class.
    Measured on the MI355X: in every class, at both lengths and with every epilogue, ALL supported tiles (all 23 at
    stride 1 and phase-decomposed; 1-3, 9-19 at direct stride 2; 2, 3, 15, 16, 17 at direct stride 4 / 5, x6 without 2 at
    stride 5) give the same bits, the register-A kernel (x6 tile 20) and the 16-byte staging included.  So the test
    asserts one equivalence class, which contains the narrow-launch set."""
    st = torch.cuda.current_stream().cuda_stream
    Cout, Cin = BITID_COUT, CIN
    for Tout, aligned in BITID_TOUT:
        xoff = 0 if aligned else 1
        Tin = in_len(cls, Tout, aligned)
        cd = case_data(cls, Cin, Cout, Tin)
        xg = _guarded(dev, (B, Cin, Tin), xoff, cd.x)
        res = cd.res.to(dev)
        sa, sb = _snake_coeffs(cd, dev)
        for epi in ("bias", "nobias", "res_snake") + (("tanh",) if cls.name == "k7" else ()):
            dual = epi == "res_snake"
            outs = {}
            for tile in range(N_X6_TILES):
                cfg = FAMILIES[family] + tile + (1000 * cls.s if cls.phase else 0)
                if not supported(cfg, cls.K, cls.s, cls.d):
                    continue
                wp, bias = cd.m.packed_as(cfg, dev)
                y = torch.full((2, B, Cout, Tout), float("nan"), device=dev)
                L.call("bc_conv1d_fwd", xg[1].data_ptr(), wp.data_ptr(), L.ptr(bias) if epi != "nobias" else None,
                       L.ptr(res) if dual else None, L.ptr(sa) if dual else None, L.ptr(sb) if dual else None,
                       y[0].data_ptr(), y[1].data_ptr() if dual else None, B, Cin, Tin, Cout, Tout, cls.K, cls.s, cls.d,
                       conv_pad(cls), int(epi == "tanh"), cfg, st)
                LAUNCHED.add(launched_name(cfg, cls.K, cls.s, cls.d, Tin, xoff))
                outs[tile] = y if dual else y[0]
                _sync(f"{family} cfg {cfg} {cls.name} Tout {Tout} {epi}")
            groups = []
            for tile, y in outs.items():
                for grp in groups:
                    if torch.equal(outs[grp[0]], y):
                        grp.append(tile)
                        break
                else:
                    groups.append([tile])
            what = f"{family} {cls.name} Tout {Tout} {epi}"
            print(f"{what}: bit-identity classes {groups}")
            assert len(outs) >= 4  # the direct stride-4 / 5 classes run on the BN = 64 tiles only
            assert bool(torch.isfinite(outs[groups[0][0]]).all()), what
            if cls.s == 1 or cls.phase:
                assert set(NARROW_SET) <= set(outs), what
            assert len(groups) == 1, f"{what}: the tiles' outputs fall into {len(groups)} bit-identity classes {groups}"


# ---------------------------------------------------------------------------------------------------------------------
# Part 2: widths no preset has, through bc_conv1d_select_cfg / _select_cfg_n
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", WIDTHS)
@pytest.mark.parametrize("mode", ["fp32", "x6", "bf16", "h3"])
def test_width_sweep(dev, mode, Cout):
    """WNConv1d.run with residual and dual Snake output at Cin = Cout (stride 1) / Cout / 2 (strided), input lengths
    T = 261 and T = 50: the library's tile choice raises nothing and meets the fp64 reference.  T = 261 is a wide launch
    (Tout > 128, bc_conv1d_select_cfg) at stride 1 and 2; at stride 4 / 5 it gives Tout = 65 / 52 and, like every T = 50
    launch, takes the narrow choice (bc_conv1d_select_cfg_n).  Widths 104..120 (seven 16-row tiles: no x6-family tile)
    and Cin < 16 run the fp32 kernel in every mode; nothing else does.  The shapes are test_conv_matrix_host's
    sweep_shapes(), whose fp32 CPU arithmetic that module checks against a quarter of the tolerance."""
    lib = L.load()
    old = L.precision_mode()
    L.set_precision(mode)
    fails = []
    try:
        for cls, Cin, _, T in sweep_shapes(Cout):
            cd = case_data(cls, Cin, Cout, T)
            m = CV.WNConv1d(Cin, Cout, kernel_size=cls.K, stride=cls.s, dilation=cls.d, padding=conv_pad(cls))
            m.load_state_dict(cd.m.state_dict())
            m.to(dev)
            what = f"{mode} {cls.name} Cout {Cout} Cin {Cin} T {T}"
            try:
                cfg = m.prepared(dev)[2]
                if cd.Tout <= 128:
                    cfg_n = lib.bc_conv1d_select_cfg_n(Cout, Cin, cls.K, cls.s, cls.d, MODES[mode], B, cd.Tout)
                    cfg = cfg_n if cfg_n >= 0 else cfg
                raw, act = m.run(cd.x.to(dev), residual=cd.res.to(dev), out_snake=_snake_coeffs(cd, dev), dual=True)
                _sync(what)
            except L.BigCodecLibraryError as e:
                fails.append(f"{what}: {e}")
                continue
            LAUNCHED.add(launched_name(cfg, cls.K, cls.s, cls.d, T, 0))
            fallback = mode == "fp32" or 104 <= Cout <= 120 or Cin < 16
            if (cfg < 100) != fallback:
                fails.append(f"{what}: cfg {cfg}, expected {'an fp32 cfg' if fallback else 'a tile of the mode'}")
            fam = "fp32" if cfg < 100 else mode
            tol = tolerance(fam, Cin, cls.K)
            want, want_act = cd.want("res_snake")
            for name, got, w, t in (("raw", raw, want, tol), ("act", act, want_act, tol * (4 if fam != "bf16" else 1))):
                got = got.cpu()
                if tuple(got.shape) != tuple(w.shape) or not bool(torch.isfinite(got).all()):
                    fails.append(f"{what} cfg {cfg}: {name} shape {tuple(got.shape)} or non-finite values")
                    continue
                err = clip_rel_err(got, w)
                if err > t:
                    fails.append(f"{what} cfg {cfg}: {name} rel err {err:.3e} > {t:.1e}")
                if fam == "bf16" and name == "raw" and err <= 1e-5:
                    fails.append(f"{what} cfg {cfg}: rel err {err:.3e}: not bf16 products")
    finally:
        L._mode = old
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


def test_ngf40_model(dev, prec):
    """The debug preset at ngf = 40 (channels 40 / 80 / 160 / 320 / 640 / 1280: the 128 x 256 tile with a partly empty
    last m-group on most convs) against the CPU oracle, 0.6 s of audio, at test_gpu_model's tolerances: latent 1e-4,
    indices equal except at certified near-ties, waveform from the oracle's z_q MSE <= 1e-12 and max <= 1e-5."""
    from audiotokenization_amd import synth

    enc, dec, esd, dsd, ek, dk = build_models("debug", device=dev, ngf=40)
    x = torch.from_numpy(synth.synth_clips(2, 9600, clip0=5)).unsqueeze(1)
    with torch.no_grad():
        lat_ref = O.encoder_forward(x, torch_sd(esd), ek)
        post_ref, codes_ref, _ = O.rvq_forward(lat_ref, torch_sd(dsd))
        ze_ref = O.fvq_forward(lat_ref, torch_sd(dsd), "quantizer.layers.0.", return_ze=True)[3]
        wav_ref = O.decoder_forward(post_ref, torch_sd(dsd), dk)
        lat = enc(x.to(dev))
        codes = dec(lat, vq=True)[1]
        wav = dec(post_ref.to(dev), vq=False)
        torch.cuda.synchronize()
    assert_close_rel(lat.cpu(), lat_ref, 1e-4, "latent")
    gap = top2_gap(ze_ref, torch.from_numpy(dsd["quantizer.layers.0._codebook.weight"]))
    n_bad, worst = index_mismatches(codes.cpu().numpy(), codes_ref.numpy(), gap)
    w, ref = wav.cpu().double(), wav_ref.double()
    assert w.shape == ref.shape
    mse, mx = float(((w - ref) ** 2).mean()), float((w - ref).abs().max())
    print(f"ngf 40 [{prec}]: {n_bad} index mismatches (worst certified gap {worst:.2e}), decoder mse {mse:.2e} max {mx:.2e}")
    assert mse <= 1e-12 and mx <= 1e-5


def test_zz_launch_set_covers_the_host_list():
    """Runs last: the instantiations launched above contain every one the host enumeration lists for a supported
    combination (so a tile or variant cannot drop out of the matrix unnoticed)."""
    want = matrix_names()
    print(f"launched {len(LAUNCHED)} distinct conv instantiations, the host list has {len(want)}:")
    for n in sorted(LAUNCHED):
        print("  " + n + ("" if n in want else "   (not in the host list)"))
    assert not want - LAUNCHED, sorted(want - LAUNCHED)
