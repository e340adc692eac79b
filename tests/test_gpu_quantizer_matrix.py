"""The quantizer kernels of csrc/vq.hip on the MI355X through the C ABI, one at a time, at every codebook size, width and
edge, against the restatement of tests/quantizer_ref.py (proved on the host by test_quantizer_host.py).

  exact:    codebook preparation, the search alone, the fused forward's indices on its own z_e, proj=False gathers,
            bc_vq2emb_ct against bc_vq2emb, bc_rvq_update, bc_fsq_codes against bc_fsq_fwd's post: bit for bit, no frame
            forgiven;
  bounded:  float outputs against float64: max|got - ref64| <= min(4 x max|ref32 - ref64|, 1e-4 x max|ref64|), the
            restatement in float32 / float64 on the same inputs (the bound of test_gpu_conformer_ops.check);
  capped:   the fused forward's indices against the torch-CPU oracle may differ only at frames whose float64 top-2 gap
            is under helpers.GAP_TOL, the FSQ indices only at frames whose float64 margin is at or under the case's
            threshold (4 x the float32 restatement's deviation in the bounded value); at most 1 % of a case's frames.

Every operand and output of a call sits between guard bands (NaN for floats, a sentinel for integers) and outputs start
as NaN / the sentinel: an element never written, a NaN where none is expected or a touched band fails the case.  After
every launch `_sync` waits for it; a device error ends the whole run."""
import numpy as np
import pytest
import torch

import quantizer_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import modules as M
from audiotokenization_amd import ops
from helpers import GAP_TOL, top2_gap
from oracle import bigcodec_oracle as O
from oracle import vq_c

pytestmark = pytest.mark.gpu

BAND = 512
F32, F64 = R.F32, R.F64
SENTINEL = {torch.int64: -(2 ** 62) - 12345, torch.int32: -(2 ** 30) - 77}


def _sync(what):
    """Wait for the launch; a device fault ends the whole run (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after {what}: {e}", returncode=3)


class Banded:
    """A contiguous device tensor of `shape` between two guard bands: float32 between NaN bands (NaN itself unless `src`
    is given), or an integer tensor (`dtype`) between bands of its sentinel (the sentinel itself unless `src` is given)."""

    def __init__(self, shape, dev, src=None, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.fill = float("nan") if dtype == torch.float32 else SENTINEL[dtype]
        self.buf = torch.full((self.n + 2 * BAND,), self.fill, device=dev, dtype=dtype)
        self.t = self.buf[BAND:BAND + self.n].view(shape)
        if src is not None:
            self.t.copy_(torch.as_tensor(src).to(dtype))
        self.ptr = self.t.data_ptr()

    def _is_fill(self, x):
        return torch.isnan(x) if self.buf.dtype == torch.float32 else x == self.fill

    def intact(self):
        return bool(self._is_fill(self.buf[:BAND]).all() and self._is_fill(self.buf[BAND + self.n:]).all())

    def untouched(self):
        return bool(self._is_fill(self.t).all())

    def written(self):
        return not bool(self._is_fill(self.t).any())

    def cpu(self):
        return self.t.detach().cpu()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def bits(x):
    """The bit patterns of a float32 array / tensor (so that -0. != +0. and NaN == NaN)."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def launch(dev, name, *args):
    L.call(name, *args, stream(dev))
    _sync(name)


def intact(*tensors):
    return all(t.intact() for t in tensors if t is not None)


def check(got, ref32, ref64, what):
    """The float64 bound on a CPU tensor `got`; prints the figures, returns err / bound."""
    got = got.double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    bound, own = R.bound(ref32, ref64)
    err = float((got - ref64).abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"QM {what}: err {err:.3e}, float32 restatement {own:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    return ratio


# ---- (a) codebook preparation ------------------------------------------------------------------------------------------
def prepare(dev, cb):
    """bc_vq_prepare_codebook on a banded codebook -> (cb, cbn, csq) banded, checked bit for bit against the C oracle."""
    n = cb.shape[0]
    ci, cbn, csq = Banded((n, 8), dev, cb), Banded((n, 8), dev), Banded((n,), dev)
    launch(dev, "bc_vq_prepare_codebook", ci.ptr, cbn.ptr, csq.ptr, n, 8)
    want_cbn, want_csq = vq_c.prepare(np.asarray(cb, np.float32))
    assert intact(ci, cbn, csq), "a guard band was written"
    assert np.array_equal(bits(cbn.t), bits(want_cbn)) and np.array_equal(bits(csq.t), bits(want_csq)), f"prepare n={n}"
    return ci, cbn, csq


@pytest.mark.parametrize("n", R.PREP_SIZES)
def test_prepare_codebook_bitwise(dev, n):
    cb, special = R.prep_codebook(n)
    _, cbn, csq = prepare(dev, cb)
    assert cbn.written() and csq.written()  # (no NaN: a zero row divides by the eps clamp)
    for name, at in special.items():
        if name.startswith("dup"):
            assert np.array_equal(bits(cbn.t[at]), bits(cbn.t[0])), name


# ---- (b) the search alone ----------------------------------------------------------------------------------------------
def run_argmin(dev, ze, prep):
    _, cbn, csq = prep
    N = ze.shape[0]
    zi, idx = Banded((N, 8), dev, ze), Banded((N,), dev, dtype=torch.int64)
    launch(dev, "bc_vq_argmin", zi.ptr, cbn.ptr, csq.ptr, idx.ptr, N, cbn.t.shape[0], 8)
    assert intact(zi, cbn, csq, idx) and idx.written()
    return idx.cpu().numpy()


@pytest.mark.parametrize("N", R.ARGMIN_ROWS)
@pytest.mark.parametrize("n", R.ARGMIN_CODES)
def test_argmin_equals_the_c_oracle_on_every_row(dev, n, N):
    cb = R.argmin_codebook(n)[0]
    ze, expect, _ = R.argmin_latents(n, N)
    got = run_argmin(dev, ze, prepare(dev, cb))
    want = vq_c.argmin(ze, cb)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"n_codes={n} N={N}: rows {bad[:8].tolist()} give {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}"
    for row, code in expect.items():  # the planted ties (the lowest copy) and the single winners
        assert got[row] == code, (row, int(got[row]), code)


@pytest.mark.parametrize("n", [1, 5, 1025, 2049, 8192])
def test_argmin_non_finite_rows_give_index_0(dev, n):
    N = 513
    cb, _, _ = R.argmin_codebook(n)
    ze, _, _ = R.argmin_latents(n, N)
    prep = prepare(dev, cb)
    plain = run_argmin(dev, ze, prep)
    ze2 = ze.copy()
    ze2[100], ze2[300] = R.nonfinite_rows()
    got = run_argmin(dev, ze2, prep)
    assert got[100] == 0 and got[300] == 0
    keep = np.ones(N, bool)
    keep[[100, 300]] = False
    assert np.array_equal(got[keep], plain[keep]) and np.array_equal(got, vq_c.argmin(ze2, cb))


# ---- (c) the fused forward ---------------------------------------------------------------------------------------------
class VQOperands:
    def __init__(self, dev, p):
        self.p = p
        self.cb, self.cbn, self.csq = prepare(dev, p["cb"].numpy())
        self.w_in, self.b_in = Banded(p["w_in"].shape, dev, p["w_in"]), Banded((8,), dev, p["b_in"])
        self.w_out, self.b_out = Banded(p["w_out"].shape, dev, p["w_out"]), Banded(p["b_out"].shape, dev, p["b_out"])

    def all(self):
        return (self.cb, self.cbn, self.csq, self.w_in, self.b_in, self.w_out, self.b_out)


def run_fwd(dev, op, zi, B, D, T, want_ze, want_post):
    idx = Banded((B, T), dev, dtype=torch.int64)
    ze = Banded((B, 8, T), dev) if want_ze else None
    post = Banded((B, D, T), dev) if want_post else None
    launch(dev, "bc_vq_fwd", zi.ptr, op.w_in.ptr, op.b_in.ptr, op.cb.ptr, op.cbn.ptr, op.csq.ptr, op.w_out.ptr, op.b_out.ptr,
           idx.ptr, ze.ptr if ze else None, post.ptr if post else None, B, D, T, op.cb.t.shape[0], 8)
    assert intact(zi, idx, ze, post, *op.all()), "a guard band was written"
    assert idx.written() and (ze is None or ze.written()) and (post is None or post.written()), "an output element was not written"
    return idx.cpu(), ze.cpu() if ze else None, post.cpu() if post else None


@pytest.mark.parametrize("D,B,T,n_codes", R.fwd_cases())
def test_fused_forward(dev, D, B, T, n_codes):
    c = R.fwd_case(D, B, T, n_codes)
    p = c["params"]
    what = f"vq_fwd D={D} B={B} T={T} n_codes={n_codes}"
    op, zi = VQOperands(dev, p), Banded((B, D, T), dev, c["z"])
    idx, ze, post = run_fwd(dev, op, zi, B, D, T, True, True)
    # z_e against float64
    check(ze, c["ze32"], c["ze64"], what + " z_e")
    # the search on the kernel's own z_e: the C oracle's index on every frame
    own = vq_c.argmin(R.rows(ze).numpy(), p["cb"].numpy()).reshape(B, T)
    assert 0 <= int(idx.min()) and int(idx.max()) < n_codes
    assert np.array_equal(idx.numpy(), own), f"{what}: {int((idx.numpy() != own).sum())} frames differ from the search on the kernel's z_e"
    # post against float64 on the kernel's indices
    check(post, R.post_of(c["ze32"], idx, p, F32), R.post_of(c["ze64"], idx, p, F64), what + " post")
    # against the torch-CPU oracle: only certified near-ties, at most 1 % of the frames
    _, o_idx, _, o_ze = O.fvq_forward(c["z"], {"in_proj.weight": p["w_in"], "in_proj.bias": p["b_in"], "_codebook.weight": p["cb"],
                                               "out_proj.weight": p["w_out"], "out_proj.bias": p["b_out"]}, "", return_ze=True)
    differ = (idx != o_idx).numpy()
    gap = top2_gap(o_ze, p["cb"])
    worst = float(gap[differ].max()) if differ.any() else 0.0
    print(f"QM {what}: {int(differ.sum())} of {B * T} frames differ from the torch-CPU oracle (largest gap {worst:.2e})")
    assert worst < GAP_TOL and differ.sum() <= R.MAX_SHARE * B * T
    # the optional outputs change nothing
    idx2, ze2, _ = run_fwd(dev, op, zi, B, D, T, True, False)
    idx3, _, post3 = run_fwd(dev, op, zi, B, D, T, False, True)
    assert torch.equal(idx2, idx) and torch.equal(idx3, idx)
    assert np.array_equal(bits(ze2), bits(ze)) and np.array_equal(bits(post3), bits(post))


# ---- (d) vq2emb --------------------------------------------------------------------------------------------------------
def run_vq2emb(dev, idx, col, stride, cb, w, b, out, N, D, n_codes, accumulate):
    launch(dev, "bc_vq2emb", idx.ptr + 8 * col, stride, cb.ptr, w.ptr if w else None, b.ptr if b else None, out.ptr, N, D,
           n_codes, 8, accumulate)
    assert intact(idx, cb, w, b, out), "a guard band was written"
    return out.cpu()


@pytest.mark.parametrize("D,N,n_codes", R.emb_cases())
def test_vq2emb_modes(dev, D, N, n_codes):
    c = R.emb_case(D, N, n_codes)
    p = c["params"]
    cb, w, b = Banded(p["cb"].shape, dev, p["cb"]), Banded(p["w_out"].shape, dev, p["w_out"]), Banded((D,), dev, p["b_out"])
    for stride in (1, 3):
        for col in range(3):
            idx = Banded((N, 3), dev, c["idx"], torch.int64) if stride == 3 else Banded((N,), dev, c["idx"][:, col], torch.int64)
            for acc in (0, 1):
                out = Banded((N, D), dev, c["base"] if acc else None)
                got = run_vq2emb(dev, idx, col if stride == 3 else 0, stride, cb, w, b, out, N, D, n_codes, acc)
                base = c["base"] if acc else None
                check(got, R.vq2emb(c["idx"], col, p["cb"], p["w_out"], p["b_out"], base, F32),
                      R.vq2emb(c["idx"], col, p["cb"], p["w_out"], p["b_out"], base, F64),
                      f"vq2emb D={D} N={N} n_codes={n_codes} stride={stride} col={col} accumulate={acc}")


@pytest.mark.parametrize("N", R.EMB_N)
@pytest.mark.parametrize("n_codes", R.EMB_CODES)
def test_vq2emb_without_projection_is_a_gather(dev, N, n_codes):
    c = R.emb_case(31, N, n_codes)
    cbt = c["params"]["cb"]
    cb = Banded(cbt.shape, dev, cbt)
    base = torch.randn(N, 8, generator=R.gen(N + n_codes))
    idx = Banded((N, 3), dev, c["idx"], torch.int64)
    for col in range(3):
        rows = cbt[c["idx"][:, col]]
        got = run_vq2emb(dev, idx, col, 3, cb, None, None, Banded((N, 8), dev), N, 8, n_codes, 0)
        assert np.array_equal(bits(got), bits(rows))
        got = run_vq2emb(dev, idx, col, 3, cb, None, None, Banded((N, 8), dev, base), N, 8, n_codes, 1)
        assert np.array_equal(bits(got), bits(base + rows))


@pytest.mark.parametrize("T", [255, 257])
@pytest.mark.parametrize("D", [31, 33])
@pytest.mark.parametrize("nq", [1, 3])
def test_vq2emb_ct_equals_vq2emb_and_a_transpose(dev, nq, D, T):
    B, n_codes = 2, 300
    g = R.gen(nq * 1000 + D * 10 + T)
    ps = [R.vq_params(D, n_codes, g) for _ in range(nq)]
    idx_t = torch.randint(0, n_codes, (B, T, nq), generator=g)
    idx_t[0, 0, :], idx_t[-1, -1, :] = 0, n_codes - 1
    idx = Banded((B, T, nq), dev, idx_t, torch.int64)
    cbs = Banded((nq, n_codes, 8), dev, torch.stack([p["cb"] for p in ps]))
    ws = Banded((nq, D, 8), dev, torch.stack([p["w_out"] for p in ps]))
    bs = Banded((nq, D), dev, torch.stack([p["b_out"] for p in ps]))
    ct = Banded((B, D, T), dev)
    launch(dev, "bc_vq2emb_ct", idx.ptr, nq, cbs.ptr, ws.ptr, bs.ptr, ct.ptr, B, T, D, n_codes, 8)
    assert intact(idx, cbs, ws, bs, ct) and ct.written()
    emb = Banded((B * T, D), dev)
    for q in range(nq):  # the same banded stacks, one quantizer's slice at a time
        L.call("bc_vq2emb", idx.ptr + 8 * q, nq, cbs.ptr + 4 * q * n_codes * 8, ws.ptr + 4 * q * D * 8, bs.ptr + 4 * q * D,
               emb.ptr, B * T, D, n_codes, 8, int(q > 0), stream(dev))
        _sync("bc_vq2emb")
    assert intact(idx, cbs, ws, bs, emb) and emb.written()
    assert np.array_equal(bits(ct.t), bits(emb.t.view(B, T, D).transpose(1, 2).contiguous()))
    # and both within the float64 bound of the looped restatement
    flat, acc32, acc64 = idx_t.reshape(-1, nq), None, None
    for q, p in enumerate(ps):
        acc32 = R.vq2emb(flat, q, p["cb"], p["w_out"], p["b_out"], acc32, F32)
        acc64 = R.vq2emb(flat, q, p["cb"], p["w_out"], p["b_out"], acc64, F64)
    check(emb.cpu(), acc32, acc64, f"vq2emb_ct nq={nq} D={D} T={T}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("proj", [True, False])
def test_vq2emb_out_of_range_index_gives_nan_not_a_read(dev, proj, accumulate):
    """Indices n_codes and -1 (the two neighbours of the codebook, as test_gpu_tokens.py's _ct test uses): their rows are
    NaN, also when accumulating; every other row is what the run with valid indices gives, bit for bit.  The codebook the
    kernel is given is the middle of a larger finite tensor, so a read at row -1 or row n_codes would return finite
    numbers (and fail this test) without leaving the allocation."""
    N, n_codes, D = 257, 5, 31 if proj else 8
    g = R.gen(99 + int(proj))
    p = R.vq_params(D, n_codes + 2, g)
    cb = Banded((n_codes + 2, 8), dev, p["cb"])
    w, b = (Banded((D, 8), dev, p["w_out"]), Banded((D,), dev, p["b_out"])) if proj else (None, None)
    base = torch.randn(N, D, generator=g)
    good = torch.randint(0, n_codes, (N, 3), generator=g)
    bad = good.clone()
    bad[3, 1], bad[200, 1], bad[256, 1] = n_codes, -1, n_codes
    outs = []
    for idx_t in (good, bad):
        idx = Banded((N, 3), dev, idx_t, torch.int64)
        out = Banded((N, D), dev, base if accumulate else None)
        launch(dev, "bc_vq2emb", idx.ptr + 8, 3, cb.ptr + 4 * 8, w.ptr if w else None, b.ptr if b else None, out.ptr, N, D,
               n_codes, 8, accumulate)
        assert intact(idx, cb, w, b, out), "a guard band was written"
        outs.append(out.cpu())
    ok = np.ones(N, bool)
    ok[[3, 200, 256]] = False
    assert not torch.isnan(outs[0]).any()
    assert torch.isnan(outs[1][~torch.from_numpy(ok)]).all(), "an out-of-range index did not give an all-NaN row"
    assert np.array_equal(bits(outs[1][ok]), bits(outs[0][ok]))


# ---- (e) rvq_update and the three-layer ResidualVQ -----------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", R.RVQ_N)
def test_rvq_update_bitwise(dev, n, first):
    r, o, q = R.rvq_case(n)
    want_r, want_o = R.rvq_update(r, o, q, first)
    ri, oi, qi = (Banded((n,), dev, torch.from_numpy(a)) for a in (r, o, q))
    if first:
        oi.t.fill_(float("nan"))  # `first` never reads out
    launch(dev, "bc_rvq_update", ri.ptr, oi.ptr, qi.ptr, n, first)
    assert intact(ri, oi, qi)
    assert np.array_equal(bits(ri.t), bits(want_r)) and np.array_equal(bits(oi.t), bits(want_o))
    assert np.array_equal(bits(qi.t), bits(q))


def test_three_layer_residual_vq_is_its_manual_composition(dev):
    D, B, T = 40, 2, 171
    g = R.gen(4242)
    rvq = M.ResidualVQ(num_quantizers=3, dim=D, codebook_size=list(R.RVQ_SIZES), codebook_dim=8, commitment=0.25)
    with torch.no_grad():
        for prm in rvq.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
    rvq.eval()
    assert [layer._codebook.weight.shape[0] for layer in rvq.layers] == list(R.RVQ_SIZES)
    folded = [{"cb": layer._codebook.weight.detach().clone(), "w_out": layer.out_proj.folded_weight().detach().clone(),
               "b_out": layer.out_proj.bias.detach().clone()} for layer in rvq.layers]
    z = torch.randn(B, D, T, generator=g) * 2.0
    rvq.to(dev)
    with torch.no_grad():
        out, idx, _ = rvq(z.to(dev))
        _sync("ResidualVQ.forward")
        residual, out2, manual = z.to(dev).clone(), torch.full_like(out, float("nan")), []
        for i, layer in enumerate(rvq.layers):
            ind, ze, q = layer.quantize(residual, want_ze=True)
            _sync("quantize")
            own = vq_c.argmin(R.rows(ze.cpu()).numpy(), folded[i]["cb"].numpy()).reshape(B, T)
            assert np.array_equal(ind.cpu().numpy(), own), f"layer {i}: the search on the kernel's own z_e"
            ops.load().rvq_update_(residual, out2, q, i == 0)
            _sync("rvq_update_")
            manual.append(ind)
        assert torch.equal(idx, torch.stack(manual)) and np.array_equal(bits(out), bits(out2))
        assert len(torch.unique(idx[1])) > 1 and int(idx[0].max()) <= 1024 and int(idx[1].max()) < 300
        vq = idx.permute(1, 2, 0).contiguous()
        emb = rvq.vq2emb(vq)
        _sync("ResidualVQ.vq2emb")
    flat, acc32, acc64 = vq.cpu().reshape(-1, 3), None, None
    for q, p in enumerate(folded):
        acc32 = R.vq2emb(flat, q, p["cb"], p["w_out"], p["b_out"], acc32, F32)
        acc64 = R.vq2emb(flat, q, p["cb"], p["w_out"], p["b_out"], acc64, F64)
    check(emb.cpu().reshape(-1, D), acc32, acc64, "ResidualVQ.vq2emb, three layers")


# ---- (f) FSQ forward -----------------------------------------------------------------------------------------------------
def fsq_operands(dev, p, levels, D):
    consts = M.FSQ(list(levels), dim=D, channel_first=True).constants()
    assert tuple(consts.shape) == (5, len(levels))
    return (Banded(p["w_in"].shape, dev, p["w_in"]), Banded(p["b_in"].shape, dev, p["b_in"]), Banded(p["w_out"].shape, dev, p["w_out"]),
            Banded(p["b_out"].shape, dev, p["b_out"]), Banded(consts.shape, dev, consts))


def run_fsq_codes(dev, idx, levels, w_out, b_out, B, D, T):
    lv = np.array(levels, np.int32)
    out = Banded((B, D, T), dev)
    launch(dev, "bc_fsq_codes", idx.ptr, 64 if idx.buf.dtype == torch.int64 else 32, lv.ctypes.data, w_out.ptr, b_out.ptr, out.ptr,
           B, D, T, len(levels))
    assert intact(idx, w_out, b_out, out) and out.written()
    return out.cpu()


@pytest.mark.parametrize("levels,D,B,T", R.fsq_cases())
def test_fsq_forward(dev, levels, D, B, T):
    c = R.fsq_case(levels, D, B, T)
    what = f"fsq_fwd levels={list(levels)} D={D} B={B} T={T}"
    w_in, b_in, w_out, b_out, consts = fsq_operands(dev, c["params"], levels, D)
    zi = Banded((B, D, T), dev, c["z"])
    idx, post = Banded((B, T), dev, dtype=torch.int32), Banded((B, D, T), dev)
    launch(dev, "bc_fsq_fwd", zi.ptr, w_in.ptr, b_in.ptr, w_out.ptr, b_out.ptr, consts.ptr, idx.ptr, post.ptr, B, D, T, len(levels))
    idx2 = Banded((B, T), dev, dtype=torch.int32)
    launch(dev, "bc_fsq_fwd", zi.ptr, w_in.ptr, b_in.ptr, None, None, consts.ptr, idx2.ptr, None, B, D, T, len(levels))
    assert intact(zi, w_in, b_in, w_out, b_out, consts, idx, idx2, post) and idx.written() and idx2.written() and post.written()
    got, gpost = idx.cpu(), post.cpu()
    assert torch.equal(got, idx2.cpu())
    differ = (got != c["idx64"]).numpy()
    ex = c["excluded"]
    print(f"QM {what}: threshold {c['threshold']:.3e}, {int(ex.sum())} of {B * T} frames under it, {int(differ.sum())} differ from float64")
    assert not differ[~ex].any(), f"{what}: frames {np.argwhere(differ & ~ex)[:4].tolist()} differ above the margin threshold"
    assert ex.sum() <= R.MAX_SHARE * B * T
    same = torch.from_numpy(~differ)[:, None, :].expand(-1, D, -1)
    check(gpost[same], c["post32"][same], c["post64"][same], what + " post")
    # the decode kernel on forward's indices gives forward's post, bit for bit
    assert np.array_equal(bits(run_fsq_codes(dev, idx, levels, w_out, b_out, B, D, T)), bits(gpost))


def test_fsq_forward_refuses_nine_levels_and_writes_nothing(dev):
    B, D, T, d = 1, 16, 4, 9
    zi, w_in, b_in = Banded((B, D, T), dev, torch.zeros(B, D, T)), Banded((d, D), dev, torch.zeros(d, D)), Banded((d,), dev, torch.zeros(d))
    w_out, b_out, consts = Banded((D, d), dev, torch.zeros(D, d)), Banded((D,), dev, torch.zeros(D)), Banded((5, d), dev, torch.ones(5, d))
    idx, post = Banded((B, T), dev, dtype=torch.int32), Banded((B, D, T), dev)
    rc = L.load().bc_fsq_fwd(zi.ptr, w_in.ptr, b_in.ptr, w_out.ptr, b_out.ptr, consts.ptr, idx.ptr, post.ptr, B, D, T, d, stream(dev))
    _sync("bc_fsq_fwd d=9")
    assert rc == 3 and idx.untouched() and post.untouched() and intact(idx, post)
    lv = np.full(d, 4, np.int32)
    rc = L.load().bc_fsq_codes(idx.ptr, 32, lv.ctypes.data, w_out.ptr, b_out.ptr, post.ptr, B, D, T, d, stream(dev))
    _sync("bc_fsq_codes d=9")
    assert rc == 3 and post.untouched()


# ---- (g) FSQ decode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.FSQ_CODES_T)
@pytest.mark.parametrize("D", R.FSQ_CODES_D)
@pytest.mark.parametrize("levels", R.FSQ_LEVELS)
def test_fsq_codes(dev, levels, D, T):
    p = R.fsq_codes_case(levels, D, T)["params"]
    w_out, b_out = Banded(p["w_out"].shape, dev, p["w_out"]), Banded(p["b_out"].shape, dev, p["b_out"])
    outs = {}
    for nbits, dtype in ((64, torch.int64), (32, torch.int32)):
        arr, fits = R.fsq_code_indices(levels, T, nbits)
        idx = Banded((1, T), dev, torch.from_numpy(arr), dtype)
        outs[nbits] = run_fsq_codes(dev, idx, levels, w_out, b_out, 1, D, T)
        check(outs[nbits], R.fsq_codes(arr, levels, p["w_out"], p["b_out"], F32), R.fsq_codes(arr, levels, p["w_out"], p["b_out"], F64),
              f"fsq_codes levels={list(levels)} D={D} T={T} int{nbits}")
    both = torch.from_numpy(fits[0])
    assert both.any() and np.array_equal(bits(outs[32][:, :, both]), bits(outs[64][:, :, both]))
