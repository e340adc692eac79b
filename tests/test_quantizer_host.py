"""The quantizer restatement (tests/quantizer_ref.py) without a GPU, before any kernel is compared with it: its float32
form equals the existing oracles (oracle/bigcodec_oracle.py: integers exactly, floats within 1e-6 of max|ref|, the bound
the VQ tests use for MKL's K = 8 order), the planted ties / non-finite rows / zero rows of the search cases do in the C
oracle and in torch's decode_latents what they are there for, every case of test_gpu_quantizer_matrix.py stays within its
cap of excluded frames from the restatements alone, and the library refuses what it does not support before any launch."""
import numpy as np
import pytest
import torch

import quantizer_ref as R
from audiotokenization_amd import _lib as L
from helpers import GAP_TOL, max_rel_err
from oracle import bigcodec_oracle as O
from oracle import vq_c

F32 = R.F32


def fvq_sd(p, prefix=""):
    return {prefix + "in_proj.weight": p["w_in"], prefix + "in_proj.bias": p["b_in"], prefix + "_codebook.weight": p["cb"],
            prefix + "out_proj.weight": p["w_out"], prefix + "out_proj.bias": p["b_out"]}


def fsq_sd(p):
    return {"quantizer.project_in.weight": p["w_in"], "quantizer.project_in.bias": p["b_in"],
            "quantizer.project_out.weight": p["w_out"], "quantizer.project_out.bias": p["b_out"]}


# ---- the restatement equals the oracles --------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,T,n_codes", R.fwd_cases())
def test_fvq_restatement_equals_the_oracle(D, B, T, n_codes):
    c = R.fwd_case(D, B, T, n_codes)
    post, idx, _, ze = O.fvq_forward(c["z"], fvq_sd(c["params"]), "", return_ze=True)
    assert torch.equal(idx, c["idx32"])
    assert max_rel_err(c["ze32"], ze) <= 1e-6 and max_rel_err(c["post32"], post) <= 1e-6
    # the float64 search is the helpers' certificate
    from helpers import top2_gap

    assert np.allclose(top2_gap(c["ze64"], c["params"]["cb"]).reshape(-1), c["gap"].reshape(-1), rtol=1e-6, atol=1e-9)


def rvq_three():
    """A three-layer ResidualVQ with codebook sizes [1025, 300, 8192] through the float32 restatement: (z, layers, post,
    idx (3, B, T))."""
    g = R.gen(777)
    D, B, T = 40, 2, 171
    layers = [R.vq_params(D, n, g) for n in R.RVQ_SIZES]
    z = torch.randn(B, D, T, generator=g) * 2.0
    residual, out, idx = z.numpy(), np.zeros_like(z.numpy()), []
    for i, p in enumerate(layers):
        _, ind, q = R.fvq(torch.from_numpy(residual), p, F32)
        residual, out = R.rvq_update(residual, out, q.numpy(), i == 0)
        idx.append(ind)
    return z, layers, torch.from_numpy(out), torch.stack(idx)


def test_rvq_restatement_equals_the_oracle():
    z, layers, post, idx = rvq_three()
    sd = {}
    for i, p in enumerate(layers):
        sd.update(fvq_sd(p, f"quantizer.layers.{i}."))
    want_post, want_idx, _ = O.rvq_forward(z, sd, "quantizer.", 3)
    assert torch.equal(idx, want_idx)
    assert max_rel_err(post, want_post) <= 1e-6
    # vq2emb: the looped sum over the three columns, and proj=False
    vq = idx.permute(1, 2, 0).contiguous()  # (B, T, 3)
    flat = vq.reshape(-1, 3)
    for proj in (True, False):
        acc = None
        for i, p in enumerate(layers):
            acc = R.vq2emb(flat, i, p["cb"], p["w_out"] if proj else None, p["b_out"] if proj else None, acc, F32)
        want = O.vq2emb(vq, sd, "quantizer.", 3, proj=proj)
        assert max_rel_err(acc.reshape(want.shape), want) <= 1e-6, proj
        if not proj:
            assert torch.equal(R.vq2emb(flat, 0, layers[0]["cb"], None, None, None, F32), layers[0]["cb"][flat[:, 0]])


@pytest.mark.parametrize("D,N,n_codes", R.emb_cases())
def test_vq2emb_restatement_equals_the_oracle(D, N, n_codes):
    c = R.emb_case(D, N, n_codes)
    p = c["params"]
    sd = fvq_sd(p, "quantizer.layers.0.")
    for col in range(3):
        got = R.vq2emb(c["idx"], col, p["cb"], p["w_out"], p["b_out"], None, F32)
        want = O.vq2emb(c["idx"][None, :, col:col + 1], sd, "quantizer.", 1)[0]
        assert max_rel_err(got, want) <= 1e-6
    assert c["seed_tries"] <= 16


@pytest.mark.parametrize("levels,D,B,T", R.fsq_cases())
def test_fsq_restatement_equals_the_oracle(levels, D, B, T):
    c = R.fsq_case(levels, D, B, T)
    p = c["params"]
    post, idx, margin = R.fsq_forward(c["z"], p["w_in"], p["b_in"], p["w_out"], p["b_out"], levels, F32)
    want_post, want_idx = O.fsq_forward(c["z"], fsq_sd(p), list(levels))
    assert want_idx.dtype == idx.dtype == torch.int32 and torch.equal(idx, want_idx)
    assert max_rel_err(post, want_post) <= 1e-6
    assert margin.dtype == torch.float64 and tuple(margin.shape) == (B, T) and 0.0 <= float(margin.min()) <= 0.5
    # the module's constant builder is the restatement's constants
    from audiotokenization_amd.modules import FSQ

    consts = FSQ(list(levels), dim=D, channel_first=True).constants()
    half_l, offset, shift, hw, basis = R.fsq_constants(levels, F32)
    assert torch.equal(consts, torch.stack([half_l, offset, shift, hw.float(), basis.float()]))
    # indices_to_codes of forward's indices, and of wrapped / negative / far integers
    got = R.fsq_codes(idx, levels, p["w_out"], p["b_out"], F32)
    assert max_rel_err(got, O.fsq_indices_to_codes(idx, fsq_sd(p), list(levels))) <= 1e-6
    assert max_rel_err(got, post) <= 1e-6


@pytest.mark.parametrize("levels", R.FSQ_LEVELS)
def test_fsq_codes_restatement_equals_the_oracle(levels):
    n = int(np.prod(levels))
    for D in R.FSQ_CODES_D:
        for T in R.FSQ_CODES_T:
            p = R.fsq_codes_case(levels, D, T)["params"]
            i64, _ = R.fsq_code_indices(levels, T, 64)
            i32, fits = R.fsq_code_indices(levels, T, 32)
            assert i64.dtype == np.int64 and i32.dtype == np.int32 and i64.shape == i32.shape == (1, T)
            assert np.array_equal(i64[fits], i32[fits].astype(np.int64))
            if T > 1:
                assert (i64 < 0).any() and (i64 >= n).any() and (np.abs(i64) > 2 ** 31).any() and not fits.all()
                assert set(range(min(n, T - 16))) <= set(i64.reshape(-1).tolist())  # every code of a small grid
            for idx in (i64, i32):
                got = R.fsq_codes(idx, levels, p["w_out"], p["b_out"], F32)
                want = O.fsq_indices_to_codes(torch.from_numpy(idx), fsq_sd(p), list(levels))
                assert max_rel_err(got, want) <= 1e-6


def test_rvq_update_restatement():
    r, o, q = R.rvq_case(257)
    r1, o1 = R.rvq_update(r, o, q, True)
    r2, o2 = R.rvq_update(r, o, q, False)
    assert np.array_equal(r1, (torch.from_numpy(r) - torch.from_numpy(q)).numpy()) and np.array_equal(r1, r2)
    assert np.array_equal(o1, (0.0 + torch.from_numpy(q)).numpy()) and np.array_equal(o2, (torch.from_numpy(o) + torch.from_numpy(q)).numpy())
    assert np.signbit(q[0]) and not np.signbit(o1[0]) and o1[0] == 0.0  # 0. + (-0.) = +0.
    assert np.signbit(o2[257 // 2])  # (-0.) + (-0.) = -0.


# ---- the planted inputs do what they are there for ---------------------------------------------------------------------
@pytest.mark.parametrize("n", R.PREP_SIZES)
def test_prepare_rows_behave_as_intended(n):
    cb, special = R.prep_codebook(n)
    cbn, csq = vq_c.prepare(cb)
    t = torch.from_numpy(cb)
    assert np.array_equal(cbn, torch.nn.functional.normalize(t).numpy())  # the C oracle is torch's F.normalize
    assert np.array_equal(csq, torch.nn.functional.normalize(t).pow(2).sum(1).numpy())
    for name, at in special.items():
        if name == "zero":
            assert not cbn[at].any() and csq[at] == 0.0
        elif name == "subnormal":
            assert 0 < abs(cb[at, 0]) < np.finfo(np.float32).tiny and np.allclose(cbn[at], 1e-28, rtol=1e-3)
        elif name == "tiny":  # the norm (2.8e-20) is under the eps clamp: divided by 1e-12, not normalised
            assert np.allclose(cbn[at], 1e-8, rtol=1e-6) and csq[at] < 1e-15
        elif name == "huge":
            assert np.isfinite(cbn[at]).all() and abs(csq[at] - 1.0) < 1e-6
        else:  # power-of-two multiples of row 0 normalise to row 0's bits
            assert np.array_equal(cbn[at], cbn[0]) and csq[at] == csq[0] and not np.array_equal(cb[at], cb[0])
    if n >= 257:
        assert set(special) == {"zero", "subnormal", "tiny", "huge", "dup_x2", "dup_x2^-20", "dup_x2^30"}


@pytest.mark.parametrize("n", R.ARGMIN_CODES)
def test_planted_search_rows_behave_as_intended(n):
    cb, plants, singles = R.argmin_codebook(n)
    cbn, csq = vq_c.prepare(cb)
    for codes in plants:  # identical bits once normalised, the lowest index first
        assert codes == sorted(codes) and all(np.array_equal(cbn[c], cbn[codes[0]]) for c in codes)
    N = 513
    ze, expect, where = R.argmin_latents(n, N)
    nan_row, inf_row = R.nonfinite_rows()
    assert not set(expect) & {100, 300} and not set(where.values()) & {100, 300}
    plain = vq_c.argmin(ze, cb)
    ze2 = ze.copy()
    ze2[100], ze2[300] = nan_row, inf_row
    c_idx = vq_c.argmin(ze2, cb)
    t_idx = O.decode_latents(torch.from_numpy(ze2.T.copy())[None], torch.from_numpy(cb))[1].reshape(-1).numpy()
    for name, idx in (("C oracle", c_idx), ("torch", t_idx)):
        for row, want in expect.items():  # a planted tie returns the lower index; the single winners win
            assert idx[row] == want, (name, n, row, int(idx[row]), want)
        assert idx[100] == 0 and idx[300] == 0, name  # all-NaN and +-Inf rows
        assert idx[where["zero"]] == int(np.argmin(csq)), name  # a zero row: the first minimum of csq
    keep = np.ones(N, bool)
    keep[[100, 300]] = False
    assert np.array_equal(c_idx[keep], plain[keep])
    # what each codebook size is there for
    last = n - ((n - 1) // R.CHUNK) * R.CHUNK
    info = {"chunks": (n + R.CHUNK - 1) // R.CHUNK, "last": last}
    if n in (2049, 4100, 8192):
        assert any(b - a == R.CHUNK for codes in plants for a, b in zip(codes, codes[1:])), info
        assert any(len(codes) == 3 for codes in plants) or n == 2049
    if n == 4100:
        assert any(codes[-1] >= 4096 for codes in plants)  # a copy in the ragged last chunk
    if n >= 5:
        assert any(codes[-1] < R.CHUNK for codes in plants)  # both copies inside one chunk
    assert singles == {"first": 0, "last": n - 1} and all(0 not in codes and n - 1 not in codes for codes in plants)
    for N_ in R.ARGMIN_ROWS:  # every launch size has the first planted row (or the last code's row) in its last block
        w = R.argmin_latents(n, N_)[2]
        assert (N_ - 1) in w.values()


# ---- the caps, from the restatements alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,T,n_codes", R.fwd_cases())
def test_fused_forward_cases_stay_within_their_cap(D, B, T, n_codes):
    c = R.fwd_case(D, B, T, n_codes)
    differ = (c["idx32"] != c["idx64"]).numpy()
    print(f"D={D} B={B} T={T} n_codes={n_codes}: {int(differ.sum())} of {B * T} frames differ between float32 and float64, "
          f"smallest gap {float(c['gap'].min()):.2e}, seed tries {c['seed_tries']}")
    assert differ.sum() <= R.MAX_SHARE * B * T
    assert not differ.any() or float(c["gap"][differ].max()) < GAP_TOL
    assert R.usable(c["ze32"], c["ze64"]) and c["seed_tries"] <= 16


@pytest.mark.parametrize("levels,D,B,T", R.fsq_cases())
def test_fsq_cases_stay_within_their_cap(levels, D, B, T):
    c = R.fsq_case(levels, D, B, T)
    ex = c["excluded"]
    print(f"levels={levels} D={D} B={B} T={T}: threshold {c['threshold']:.3e}, {int(ex.sum())} of {B * T} frames under it, "
          f"seed tries {c['seed_tries']}")
    assert ex.sum() <= R.MAX_SHARE * B * T and not ex.all()
    assert torch.equal(c["idx32"][torch.from_numpy(~ex)], c["idx64"][torch.from_numpy(~ex)])
    assert 0.0 < c["threshold"] < 1e-4 and c["seed_tries"] <= 16  # (1e-4: the margin test_gpu_fsq.py forgives)
    assert len(torch.unique(c["idx64"])) >= min(B * T, 2)


# ---- refusals that need no launch --------------------------------------------------------------------------------------
def test_the_library_refuses_before_any_launch():
    lib = L.load()
    one = 1  # a non-null pointer that is never dereferenced: every call below returns before a launch
    assert lib.bc_vq_prepare_codebook(one, one, one, 16, 4, None) == 3
    assert lib.bc_vq_fwd(one, one, one, one, one, one, one, one, one, one, one, 1, 16, 4, 16, 16, None) == 3
    assert lib.bc_vq_argmin(one, one, one, one, 4, 16, 7, None) == 3
    assert lib.bc_vq2emb(one, 1, one, one, one, one, 4, 16, 16, 9, 0, None) == 3
    assert lib.bc_vq2emb_ct(one, 1, one, one, one, one, 1, 4, 16, 16, 16, None) == 3
    for n_codes in (0, -1):
        assert lib.bc_vq_prepare_codebook(one, one, one, n_codes, 8, None) == 1
        assert lib.bc_vq_fwd(one, one, one, one, one, one, one, one, one, one, one, 1, 16, 4, n_codes, 8, None) == 1
        assert lib.bc_vq_argmin(one, one, one, one, 4, n_codes, 8, None) == 1
        assert lib.bc_vq2emb(one, 1, one, one, one, one, 4, 16, n_codes, 8, 0, None) == 1
        assert lib.bc_vq2emb_ct(one, 1, one, one, one, one, 1, 4, 16, n_codes, 8, None) == 1
    assert lib.bc_vq2emb(one, 1, one, None, None, one, 4, 16, 16, 8, 0, None) == 1  # proj=False needs D == dim
    assert lib.bc_fsq_fwd(one, one, one, one, one, one, one, one, 1, 16, 4, 9, None) == 3
    assert lib.bc_fsq_fwd(one, one, one, one, one, one, one, one, 1, 16, 4, 0, None) == 1
    lv9 = np.full(9, 4, np.int32)
    assert lib.bc_fsq_codes(one, 32, lv9.ctypes.data, one, one, one, 1, 16, 4, 9, None) == 3
    for bad in ([4, 1, 4], [0], [4, -3]):
        lv = np.array(bad, np.int32)
        assert lib.bc_fsq_codes(one, 32, lv.ctypes.data, one, one, one, 1, 16, 4, len(bad), None) == 1
    assert lib.bc_fsq_codes(one, 16, lv9.ctypes.data, one, one, one, 1, 16, 4, 4, None) == 1  # index width
    assert lib.bc_abi_version() == L.ABI_VERSION == 18  # the vq2emb range check changed no signature
