"""The bidirectional ResLSTM (bc_reslstm_bidir_fwd) against fp64 on the MI355X, on the recurrence's own output.

Everything but the raw-call test goes through blocks.ResLSTM(D, layers, bidirectional=True).run.  Cases, the fp64
reference (torch.nn.LSTM(bidirectional=True), one per case, shared by every precision and launch size: clips are
independent, so a launch of n clips is compared with ref[:n]), the metric rel_h on got - x -- for the whole output and
for each channel half (direction) -- and the bound K[prec] * cpu32 come from tests/lstm_ref.py;
tests/test_lstm_matrix_host.py::test_bidir_bound_discriminates shows on the CPU that the bound sits three orders of
magnitude below a single-plane operand in either direction's W_hh or h, or in the reverse-half columns of W_ih.  What
exists in the bidirectional call only: an input projection with Cin = 2H, time_reverse_kernel (16-byte path when
B % 4 == 0, scalar otherwise), the concatenation [forward | reverse], the persistent kernel twice per layer on one
workspace, and that workspace's carve-up.

  test_bidir                  D in {512, 1024, 2048, 3072} x {x6, h3} x n in {1, 3, 4, 63, 64, 65, 70}; for n <= 64 the
                              launch timer must have recorded lstm_seq2_x6_kernel<H / 128, P, NTH> 2 x layers times
  test_bidir_step_kernels     D = 96, 256, 1536 in fp32 mode, 1536 (H = 768: lstm_step_kernel in every mode) also in x6
  test_bidir_fp32_mode        D = 512, 2048: lstm_step_frag_kernel in both directions
  test_bidir_t_edges          T = 1, T = 2 and T = 33 (the transposes' second 32-step tile) with fp64 references of their own
  test_bidir_fused_output_snake   the Snake fused into the output transpose: against fp64, and bit for bit ops.snake(run(x))
  test_bidir_mirror_identity  exact: exchanging the directions' parameters and reversing time mirrors the output
  test_bidir_raw_call_exact_workspace   the raw calls (bidirectional and unidirectional) on a workspace of exactly the
                              reported size between NaN guard bands
  the module's last test checks that the timer saw all 16 persistent instantiations."""
import functools

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import blocks as BL
from audiotokenization_amd import modules as M
from audiotokenization_amd import ops
from lstm_ref import (BIDIR_SEQ_D, K, bidir_case, bound, cpu32, data, main_case, ref64, rel_h_halves, scales,
                      torch_lstm, worst)
from oracle import bigcodec_oracle as O
from test_gpu_lstm_matrix import _host, _module as _uni_module, _precision, _seq_name

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 63, 64, 65, 70)  # one clip; time_reverse's scalar / 16-byte path; the 64-clip tile and launch chunk
LAUNCHED = set()  # persistent instantiations the launch timer recorded, checked by the module's last test
GUARD = 512
NAN_BITS = 0x7FC00000


@pytest.fixture(autouse=True)
def _no_timed_out_wait(dev):
    yield
    assert L.load().bc_lstm_status(1) == 0


def _params(D, layers, swapped):
    """The D's parameters (every case of one D shares them), optionally with the two directions exchanged."""
    p = {k: v for k, v in data(bidir_case(D)).params.items() if int(k.split("_l")[1][0]) < layers}
    if swapped:
        p = {(k[:-len("_reverse")] if k.endswith("_reverse") else k + "_reverse"): v for k, v in p.items()}
    return p


@functools.lru_cache(maxsize=None)
def _module(D, layers=2, swapped=False):
    m = BL.ResLSTM(D, num_layers=layers, bidirectional=True)
    m.lstm.load_state_dict(_params(D, layers, swapped))
    return m.to(torch.device("cuda", 0))


def _run(dev, m, prec, x, what, out_snake=None, timed=False):
    """ResLSTM.run under a precision: (y on the host, {kernel: launches} recorded by the launch timer)."""
    tm = L.KernelTimer() if timed else None
    with _precision(prec):
        if timed:
            L.set_timer(tm)
        try:
            with L.status_scope():
                y = m.run(x.contiguous().to(dev), out_snake=out_snake)
                L.check_status()
        finally:
            if timed:
                L.set_timer(None)
    y, = _host(what, y)
    return y, ({k: d["launches"] for k, d in tm.summary().items()} if timed else {})


def _check(fails, got, want, case, prec, what, bcase=None):
    """rel_h of a slice of the case on the whole case's scale, whole and per channel half; prints the figures and their
    ratio to the fp32 CPU error, then collects a failure.  bcase: the case whose bound and scale apply
    when they are not the reference's own."""
    bcase = bcase or case
    lim, c32 = bound(bcase, prec), max(cpu32(bcase))
    e, ef, er = rel_h_halves(got, want, scales(bcase)[0])
    print(f"LSTM-MATRIX bidir {what}: rel_h {e:.3e} (fwd {ef:.3e} rev {er:.3e}) cpu32 {c32:.3e} ratio {e / c32:.2f} "
          f"(fwd {ef / c32:.2f} rev {er / c32:.2f}) bound {lim:.3e}")
    if not torch.isfinite(got).all() or e > lim:
        fails.append(f"{what}: rel_h {e:.3e} (fwd {ef:.3e} rev {er:.3e}) > {lim:.3e}; {worst(got, want, bidir=True)}")


def _leg(dev, key, prec, n, what, timed=False):
    case = bidir_case(key)
    x, ref = data(case).x[:n], ref64(case)[0][:n]
    y, names = _run(dev, _module(case.D), prec, x, what, timed=timed)
    fails = []
    _check(fails, y - x, ref, case, prec, what)
    return case, names, fails


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("D", BIDIR_SEQ_D)
def test_bidir(dev, D, prec, n):
    """The persistent kernel in both directions of both layers, on one shared workspace with a time reversal between."""
    case, names, fails = _leg(dev, D, prec, n, f"persistent D {D} {prec} n {n}", timed=n <= 64)
    if n <= 64:  # above 64 the recorded name is the first chunk's only
        name = _seq_name(case.H, prec, n)
        assert names.get(name) == 2 * case.layers, (name, names)
        LAUNCHED.add(name)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [1, 3, 64, 65])
@pytest.mark.parametrize("D,prec", [(96, "fp32"), (256, "fp32"), (1536, "fp32"), (1536, "x6")])
def test_bidir_step_kernels(dev, D, prec, n):
    """lstm_step_kernel (H = 48, 768) and lstm_step_frag_kernel<4> (H = 128), one launch per step and direction; H = 768
    has no persistent kernel, so only the projection changes between fp32 mode and x6."""
    fails = _leg(dev, D, prec, n, f"step D {D} {prec} n {n}")[2]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [4, 65])
@pytest.mark.parametrize("D", [512, 2048])
def test_bidir_fp32_mode(dev, D, n):
    fails = _leg(dev, D, "fp32", n, f"fp32 D {D} n {n}")[2]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("prec", ["x6", "h3"])
def test_bidir_t_edges(dev, prec):
    """T = 1 (the reversal is the identity, nothing is published), T = 2, and "512L" (T = 33: the transposes cross their
    32-step tile inside an fp64 leg).  A bidirectional prefix is not its own answer: T = 1 and T = 2 are cases of their
    own, D = 512's parameters on an x of their own, each with its fp64 reference.  Their errors are held to D = 512's
    bound on D = 512's scale: the same parameters run fewer steps of the same recurrence, and the fp32 error of a
    70-clip, one- or two-step sample (printed) would be a noisier, smaller yardstick than the bound's own case."""
    fails = []
    for key, T in ((512, 1), (512, 2), ("512L", None)):
        case = bidir_case(key, T=T)
        for n in (3, 4):
            x, ref = data(case).x[:n], ref64(case)[0][:n]
            what = f"T edge D 512 {prec} T {case.T} n {n}"
            y = _run(dev, _module(512), prec, x, what)[0]
            if T is not None:
                print(f"(own scale {scales(case)[0]:.3f}, own cpu32 {max(cpu32(case)):.3e})")
            _check(fails, y - x, ref, case, prec, what, bcase=bidir_case(512) if T is not None else None)
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=None)
def _snake_case(D, n):
    """Snake parameters, the fp64 Snake of x + h and the fp32 CPU pipeline's error, on the recurrence's scale."""
    case = bidir_case(D)
    g = torch.Generator().manual_seed(D + 1)
    alpha, beta = torch.rand(D, generator=g) - 0.5, torch.rand(D, generator=g) - 0.5
    x, r = data(case).x[:n], ref64(case)[0][:n]
    want = O.snake_beta(x.double() + r, alpha.double(), beta.double())
    y32 = torch_lstm(case, torch.float32)[0][:n]
    s32 = O.snake_beta(y32 + x, alpha, beta)
    scale = scales(case)[0]
    return alpha, beta, want, scale, float((s32.double() - want).abs().max()) / scale


@pytest.mark.parametrize("D,prec", [(512, "x6"), (96, "fp32")])
def test_bidir_fused_output_snake(dev, D, prec):
    """The Snake fused into the bidirectional call's output transpose: max |got - snake64(x + h64)| / max |h64| within
    K[prec] times the same figure of the fp32 CPU pipeline (tests/test_gpu_lstm_matrix.py::test_fused_output_snake), and
    bit for bit the standalone Snake of the unfused result: ctb_to_btc_add_kernel calls snake(), which
    csrc/bc_common.h states rounds exactly as snake_kernel's pairs (same operations, same order, no contraction)."""
    n = 33
    case = bidir_case(D)
    alpha, beta, want, scale, c32 = _snake_case(D, n)
    s = M.SnakeBeta(D, alpha_logscale=True)
    with torch.no_grad():
        s.alpha.copy_(alpha)
        s.beta.copy_(beta)
    coeffs = s.to(dev).coeffs(dev)
    x = data(case).x[:n]
    y = _run(dev, _module(D), prec, x, f"snake D {D} {prec}", out_snake=coeffs)[0]
    e = float((y.double() - want).abs().max()) / scale
    lim = K[prec] * c32
    print(f"LSTM-MATRIX bidir snake D {D} {prec} n {n}: rel_h {e:.3e} cpu32 {c32:.3e} ratio {e / c32:.2f} bound {lim:.3e}")
    assert torch.isfinite(y).all() and e <= lim, (e, lim, worst(y, want, bidir=True))
    with _precision(prec), L.status_scope():
        plain = _module(D).run(x.to(dev))
        L.check_status()
        two, = _host("the standalone snake", ops.load().snake(plain, *coeffs))
    assert torch.equal(two.view(torch.int32), y.view(torch.int32)), \
        (float((two - y).abs().max()), worst(y, two.double(), bidir=True))


def _flip_swap(y):
    """Time reversed, channel halves exchanged."""
    H = y.shape[1] // 2
    return torch.cat([y[:, H:], y[:, :H]], dim=1).flip(2)


@pytest.mark.parametrize("T", [7, 33])
@pytest.mark.parametrize("B", [3, 4])
def test_bidir_mirror_identity(dev, B, T):
    """Reversal and concatenation without arithmetic.  One layer, D = 512, x with equal channel halves; m' is m with the
    forward and reverse parameters exchanged.  Then m'(flip_t(x)) is flip_t(m(x)) with its channel halves exchanged:
    m' forward reads flip_t(x), the matrix m's reverse direction builds with time_reverse_kernel, at the same column
    positions, and m' reverse reads flip_t(flip_t(x)) = x; the same projection and recurrence run on the same columns
    in the same K order, only the buffers and the output positions move, and the equal halves make the residual add the
    same.  Required bit for bit of x6 (whose results are documented not to depend on the column tile); h3 and fp32 mode
    print their largest difference and, where it is not zero, both sides are held to the fp64 bound (DESIGN.md §19 has
    the outcome)."""
    case = bidir_case(512, T=T, layers=1, mirror=True)
    x = data(case).x[:B]
    assert torch.equal(x[:, :256], x[:, 256:])
    fails = []
    for prec in ("x6", "h3", "fp32"):
        what = f"mirror D 512 {prec} B {B} T {T}"
        a = _run(dev, _module(512, 1), prec, x, what)[0]
        b = _run(dev, _module(512, 1, True), prec, x.flip(2), what + " exchanged")[0]
        diff = float((_flip_swap(a) - b).abs().max())
        same = torch.equal(_flip_swap(a).view(torch.int32), b.view(torch.int32))
        print(f"LSTM-MATRIX bidir {what}: largest difference {diff:.3e}, bit-identical {same}")
        if prec == "x6":
            if not same:
                fails.append(f"{what}: differs by {diff:.3e}; {worst(b, _flip_swap(a).double(), bidir=True)}")
            _check(fails, a - x, ref64(case)[0][:B], case, prec, what)
        elif not same:
            _check(fails, a - x, ref64(case)[0][:B], case, prec, what)
            _check(fails, _flip_swap(b) - x, ref64(case)[0][:B], case, prec, what + " exchanged")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# the raw calls on a workspace of exactly the reported size


def _guarded(dev, n, src=None):
    """n floats, 16-byte aligned, NaN-filled (or a copy of src), between NaN bands of GUARD floats."""
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=dev)
    view = buf[GUARD:GUARD + n]
    assert view.data_ptr() % 16 == 0
    if src is not None:
        view.copy_(src.reshape(-1))
    return buf, view, buf.data_ptr() + 4 * GUARD  # (the pointer spelled out: an empty view still gets a valid one)


def _bands_intact(g):
    bits = g[0].view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + g[1].numel():] == NAN_BITS).all())


def _raw(dev, m, bidir, prec, x, fails, what):
    """One raw bc_reslstm[_bidir]_fwd call on guarded x, out and exact-size workspace; returns out (host) or None."""
    lib = L.load()
    B, C, T = x.shape
    with _precision(prec):
        (wih, whh, bias), arrs = m.lstm.prepared(dev)
        if bidir:
            nws = lib.bc_reslstm_bidir_workspace_floats(B, C, T)
        else:
            nws = lib.bc_lstm_workspace_floats(B, C, T)
        assert nws >= 64, nws
        xg, og, wg = _guarded(dev, x.numel(), x.to(dev)), _guarded(dev, x.numel()), _guarded(dev, nws)
        st = torch.cuda.current_stream().cuda_stream
        rc = getattr(lib, "bc_reslstm_bidir_fwd" if bidir else "bc_reslstm_fwd")(
            xg[2], og[2], B, C, T, m.lstm.num_layers, arrs[0], arrs[1], arrs[2], None, None,
            wg[2], L.precision_mode(), st)
    out, ws0, rest, xb = _host(what, og[1], wg[1][:1].view(torch.int32), wg[1][1:].view(torch.int32), xg[1])
    if rc != 0:
        fails.append(f"{what}: returned {rc}")
    if not (_bands_intact(xg) and _bands_intact(og) and _bands_intact(wg)):
        fails.append(f"{what}: a guard band was written (x {_bands_intact(xg)}, out {_bands_intact(og)}, workspace of "
                     f"exactly {nws} floats {_bands_intact(wg)})")
    if int(ws0[0]) != 0:
        fails.append(f"{what}: workspace[0] (the call's timeout count) is {int(ws0[0])}")
    if not torch.equal(xb.view(torch.int32), x.reshape(-1).view(torch.int32)):
        fails.append(f"{what}: x was written")
    if x.numel() == 0 or B == 0 or T == 0:
        if not bool((rest == NAN_BITS).all()) or not bool((og[0].view(torch.int32) == NAN_BITS).all()):
            fails.append(f"{what}: an empty call wrote more than its timeout count")
        return None
    return out.view(B, C, T)


@pytest.mark.parametrize("prec", ["x6", "fp32"])
def test_bidir_raw_call_exact_workspace(dev, prec):
    """bc_reslstm_bidir_fwd at D = 512 with x, out and a workspace of exactly bc_reslstm_bidir_workspace_floats(B, D, T)
    floats between NaN bands, workspace and out pre-filled with NaN: bit for bit the op's result (whose workspace comes
    from the caching allocator, where an overrun of the carve-up is silent), no NaN in out, every band intact, the
    timeout count 0; B = 0 and T = 0 return 0 and write nothing but that count.  The same for bc_reslstm_fwd with
    bc_lstm_workspace_floats at H = 256."""
    fails = []
    case = bidir_case(512)
    for B, T in ((3, 5), (65, 2)):
        x = data(case).x[:B, :, :T].contiguous()
        what = f"raw bidir D 512 {prec} B {B} T {T}"
        got = _raw(dev, _module(512), True, prec, x, fails, what)
        want = _run(dev, _module(512), prec, x, what)[0]
        if not torch.isfinite(got).all():
            fails.append(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs")
        elif not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            fails.append(f"{what}: differs from the op by {float((got - want).abs().max()):.3e}; "
                         f"{worst(got, want.double(), bidir=True)}")
    for B, T in ((0, 5), (3, 0)):
        _raw(dev, _module(512), True, prec, data(case).x[:B, :, :T].contiguous(), fails, f"raw bidir {prec} B {B} T {T}")
    ucase = main_case(256)
    B, T = (3, 5) if prec == "x6" else (65, 2)
    x = data(ucase).x[:B, :, :T].contiguous()
    what = f"raw unidirectional H 256 {prec} B {B} T {T}"
    got = _raw(dev, _uni_module(256), False, prec, x, fails, what)
    with _precision(prec), L.status_scope():
        want = _uni_module(256).run(x.to(dev))
        L.check_status()
    want, = _host(what, want)
    if not torch.isfinite(got).all() or not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        fails.append(f"{what}: differs from the op by {float((got - want).abs().max()):.3e}")
    for B, T in ((0, 5), (3, 0)):
        _raw(dev, _uni_module(256), False, prec, data(ucase).x[:B, :, :T].contiguous(), fails,
             f"raw unidirectional {prec} B {B} T {T}")
    assert not fails, "\n".join(fails)


def test_every_persistent_instantiation_ran_bidirectionally():
    want = {_seq_name(D // 2, prec, n) for D in BIDIR_SEQ_D for prec in ("x6", "h3") for n in (32, 33)}
    assert len(want) == 16 and LAUNCHED == want, sorted(want - LAUNCHED)
