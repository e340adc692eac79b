"""The quantizer kernels of csrc/vq.hip restated plainly on the CPU, in float32 and in float64, and the case lists the
host module (test_quantizer_host.py) and the GPU module (test_gpu_quantizer_matrix.py) share.

Written from csrc/vq.hip's header comment, oracle/bigcodec_oracle.py and oracle/vq_oracle.c.  Layouts are the kernels':
latents (B, D, T), projected latents z_e (B, 8, T), codebook (n_codes, 8), in_proj weight (8, D), out_proj weight (D, 8).
Every function takes a `dtype` (torch.float32 / torch.float64) and computes in it from start to end.

A case's inputs are a function of its shape alone (its seed is derived from the shape), except where the float32
restatement alone makes a seed unusable (see `usable`): then the next seed is taken.  Nothing here looks at a kernel."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vq_c

DIM = 8
CHUNK = 1024  # csrc/vq.hip VQ_CHUNK
F32, F64 = torch.float32, torch.float64


def _t(x, dtype):
    return torch.as_tensor(x).to(dtype)


# ---- factorized VQ ---------------------------------------------------------------------------------------------------
def in_proj(z, w, b, dtype):
    """z (B, D, T), w (8, D), b (8) -> z_e (B, 8, T) = w z + b per frame."""
    return F.linear(_t(z, dtype).transpose(1, 2), _t(w, dtype), _t(b, dtype)).transpose(1, 2).contiguous()


def out_proj(zq, w, b, dtype):
    """zq (..., 8), w (D, 8), b (D) -> (..., D)."""
    return F.linear(_t(zq, dtype), _t(w, dtype), _t(b, dtype))


def rows(z_e):
    """(B, 8, T) -> (B*T, 8), frame n = b*T + t."""
    return z_e.permute(0, 2, 1).reshape(-1, z_e.shape[1])


def search64(ze_rows, cb):
    """decode_latents' search in float64 -> (first argmin (N,), top-2 distance gap (N,); inf for a one-code codebook)."""
    e = _t(ze_rows, F64)
    c = _t(cb, F64)
    e = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)
    dist = (e * e).sum(1, keepdim=True) - 2 * e @ c.t() + (c * c).sum(1)[None]
    idx = torch.argmin(dist, dim=1)  # (ties: certified by the gap, which is 0 there)
    if dist.shape[1] == 1:
        return idx.numpy(), np.full(dist.shape[0], np.inf)
    v, _ = torch.topk(dist, 2, dim=1, largest=False)
    return idx.numpy(), (v[:, 1] - v[:, 0]).numpy()


def fvq(z, params, dtype):
    """FactorizedVectorQuantize.forward (eval): (z_e (B, 8, T), idx (B, T) int64, post (B, D, T)).  The float32 search is
    the C oracle's (oracle/vq_c.py), the float64 one search64."""
    z_e = in_proj(z, params["w_in"], params["b_in"], dtype)
    B, _, T = z_e.shape
    if dtype == F32:
        idx = vq_c.argmin(rows(z_e).numpy(), np.asarray(params["cb"], np.float32))
    else:
        idx = search64(rows(z_e), params["cb"])[0]
    idx = torch.from_numpy(np.asarray(idx, np.int64)).reshape(B, T)
    return z_e, idx, post_of(z_e, idx, params, dtype)


def post_of(z_e, idx, params, dtype):
    """out_proj of the straight-through value z_e + (codebook[idx] - z_e): (B, D, T)."""
    ze = _t(z_e, dtype).permute(0, 2, 1)
    zq = _t(params["cb"], dtype)[idx]
    st = ze + (zq - ze)
    return out_proj(st, params["w_out"], params["b_out"], dtype).permute(0, 2, 1).contiguous()


def vq2emb(idx, column, cb, w, b, accumulate_into, dtype):
    """FactorizedVectorQuantize.vq2emb on column `column` of idx (N, Nq): (N, D); w None is proj=False (codebook rows);
    accumulate_into (N, D) is added to (ResidualVQ.vq2emb's running sum)."""
    emb = _t(cb, dtype)[torch.as_tensor(idx)[:, column]]
    if w is not None:
        emb = out_proj(emb, w, b, dtype)
    return emb if accumulate_into is None else _t(accumulate_into, dtype) + emb


def rvq_update(residual, out, q, first):
    """ResidualVQ bookkeeping, float32 elementwise: (residual - q, 0. + q if first else out + q)."""
    residual, out, q = (np.asarray(a, np.float32) for a in (residual, out, q))
    return residual - q, (np.float32(0.0) + q) if first else out + q


# ---- FSQ -------------------------------------------------------------------------------------------------------------
def fsq_constants(levels, dtype):
    lv = torch.tensor(list(levels), dtype=torch.int64)
    half_l = ((lv - 1).to(dtype) * (1 + 1e-3) / 2)
    offset = torch.where(lv % 2 == 0, 0.5, 0.0).to(dtype)
    shift = torch.atanh(offset / half_l)
    basis = torch.cumprod(torch.tensor([1] + list(levels[:-1]), dtype=torch.int64), 0)
    return half_l, offset, shift, (lv // 2), basis


def fsq_bounded(z, w_in, b_in, levels, dtype):
    """(B, T, d): project_in, then bound()."""
    half_l, offset, shift, _, _ = fsq_constants(levels, dtype)
    x = F.linear(_t(z, dtype).transpose(1, 2), _t(w_in, dtype), _t(b_in, dtype))
    return torch.tanh(x + shift) * half_l - offset


def fsq_forward(z, w_in, b_in, w_out, b_out, levels, dtype):
    """FSQ.forward (eval, channel_first, one codebook): (post (B, D, T), idx (B, T) int32, margin (B, T)); margin is the
    float64 distance of the nearest bounded coordinate of the frame to a rounding boundary (x.5)."""
    _, _, _, hw, basis = fsq_constants(levels, dtype)
    bounded = fsq_bounded(z, w_in, b_in, levels, dtype)
    q = bounded + (torch.round(bounded) - bounded)
    codes = q / hw.to(dtype)
    idx = ((codes * hw.to(dtype) + hw.to(dtype)) * basis.to(dtype)).sum(-1).to(torch.int32)
    post = F.linear(codes, _t(w_out, dtype), _t(b_out, dtype)).transpose(1, 2).contiguous()
    b64 = bounded if dtype == F64 else fsq_bounded(z, w_in, b_in, levels, F64)
    margin = ((b64 - b64.floor()) - 0.5).abs().amin(dim=-1)
    return post, idx, margin


def fsq_codes(idx, levels, w_out, b_out, dtype):
    """FSQ.indices_to_codes: idx (B, T) any integer -> project_out(codes) (B, D, T); int64 floor-div / floor-mod."""
    _, _, _, hw, basis = fsq_constants(levels, dtype)
    lv = torch.tensor(list(levels), dtype=torch.int64)
    k = torch.as_tensor(idx).to(torch.int64)[..., None]
    level = torch.remainder(torch.div(k, basis, rounding_mode="floor"), lv)
    codes = (level - hw).to(dtype) / hw.to(dtype)
    return F.linear(codes, _t(w_out, dtype), _t(b_out, dtype)).transpose(1, 2).contiguous()


# ---- bounds and the seed rule ----------------------------------------------------------------------------------------
def bound(ref32, ref64):
    """(bound, own): min(4 x max|ref32 - ref64|, 1e-4 x max|ref64|), the bound of test_gpu_conformer_ops.check."""
    own = float((_t(ref32, F64) - _t(ref64, F64)).abs().max())
    return min(4.0 * own, 1e-4 * float(_t(ref64, F64).abs().max())), own


def usable(ref32, ref64):
    """A seed is usable for a float64-bound check when the float32 restatement's own error is at least a quarter of a
    float32 ulp of the output's largest magnitude (2^-25 x max|ref64|): below that, 4 x own is under one rounding of the
    result, a bound no float32 evaluation in another order can be held to (it bites only on outputs of a few elements,
    where the maximum of the restatement's error is a sample of one)."""
    own = float((_t(ref32, F64) - _t(ref64, F64)).abs().max())
    return own >= 2.0 ** -25 * float(_t(ref64, F64).abs().max())


def _first_usable(make, base, tries=64):
    for k in range(tries):
        case = make(base + 7919 * k)
        if case is not None:
            case["seed_tries"] = k + 1
            return case
    raise AssertionError("no usable seed")


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- (a) codebook preparation ----------------------------------------------------------------------------------------
PREP_SIZES = (1, 2, 255, 256, 257, 1000, 1024, 1025)


def prep_codebook(n):
    """Random rows in [-1, 1), then (where n has room): an all-zero row, a subnormal row, a 1e-20 row (its norm under the
    eps clamp), a 1e18 row, and power-of-two multiples of row 0 (they normalise to row 0's bits).  Returns (codebook,
    {name: row index})."""
    rng = np.random.default_rng(1000 + n)
    cb = (rng.random((n, DIM), dtype=np.float32) * 2 - 1).astype(np.float32)
    special = {}
    plan = [("zero", np.zeros(DIM, np.float32)), ("subnormal", np.full(DIM, 1e-40, np.float32)),
            ("tiny", np.full(DIM, 1e-20, np.float32)), ("huge", np.full(DIM, 1e18, np.float32) * np.sign(cb[0] + 0.5)),
            ("dup_x2", cb[0] * np.float32(2.0)), ("dup_x2^-20", cb[0] * np.float32(2.0 ** -20)),
            ("dup_x2^30", cb[0] * np.float32(2.0 ** 30))]
    for i, (name, row) in enumerate(plan):
        at = n - 1 - i  # from the end: the last rows sit in the ragged last block of the launch
        if at >= 1:
            cb[at] = row
            special[name] = at
    if n == 1:
        cb[0] = 0.0
        special["zero"] = 0
    return cb, special


# ---- (b) search alone ------------------------------------------------------------------------------------------------
ARGMIN_CODES = (1, 2, 3, 5, 255, 257, 1023, 1024, 1025, 2049, 4100, 8192)
ARGMIN_ROWS = (1, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def argmin_codebook(n):
    """A random codebook with planted exact ties: (codebook, plants, singles).  plants: lists of code indices holding the
    same direction (an exact copy or a power-of-two multiple of the first: identical bits once normalised), the lowest
    first; singles: {"first": 0, "last": n - 1}, codes in no plant (each the unique winner for its own row)."""
    rng = np.random.default_rng(2000 + n)
    cb = (rng.random((n, DIM), dtype=np.float32) * 2 - 1).astype(np.float32)
    want = [([1, 3], [2.0]),  # both copies inside one chunk (n >= 5)
            ([9, 100], [1.0]),  # an exact duplicate inside one chunk
            ([7, 200], [0.5]),
            ([17, 17 + CHUNK, 17 + 2 * CHUNK], [4.0, 0.25]),  # carried from one LDS pass to the next, and the one after
            ([1000, 1000 + CHUNK], [1.0])]
    last_chunk0 = ((n - 1) // CHUNK) * CHUNK
    if n - 2 > last_chunk0 and n > CHUNK:  # a copy in the ragged (or last) chunk of a many-chunk codebook
        want.append(([50, n - 2], [8.0]))
    plants, used = [], {0, n - 1}
    for codes, scales in want:
        codes = [c for c in codes if c < n - 1]
        if len(codes) < 2 or used & set(codes):
            continue
        for c, s in zip(codes[1:], scales):
            cb[c] = cb[codes[0]] * np.float32(s)
        used |= set(codes)
        plants.append(codes)
    return cb, plants, {"first": 0, "last": n - 1}


@functools.lru_cache(maxsize=None)
def argmin_latents(n, N):
    """(z_e rows (N, 8), {row: expected index}, {name: row}) for argmin_codebook(n): random rows of mixed magnitudes, and
    written over them, as far as N has room (alternately from the end, the launch's ragged last block, and from the
    start): each planted row itself and a 1e15 multiple of its last copy, the single winners, a zero, a subnormal and a
    1e-20 row, and random rows scaled by 1e+-15."""
    cb, plants, singles = argmin_codebook(n)
    rng = np.random.default_rng(3000 + 17 * n + N)
    ze = (rng.standard_normal((N, DIM)) * rng.lognormal(size=(N, 1))).astype(np.float32)
    r0 = ze[0].copy()
    special = []
    for codes in plants:
        special.append((f"tie{codes[0]}", cb[codes[0]].copy(), codes[0]))
        special.append((f"tie{codes[0]}x1e15", cb[codes[-1]] * np.float32(1e15), codes[0]))
    special += [("last", cb[singles["last"]] * np.float32(3.0), singles["last"]),
                ("first", cb[singles["first"]] * np.float32(1e-15), singles["first"]),
                ("zero", np.zeros(DIM, np.float32), None), ("subnormal", np.full(DIM, 1e-40, np.float32), None),
                ("tiny", np.full(DIM, -1e-20, np.float32), None), ("x1e15", r0 * np.float32(1e15), None),
                ("x1e-15", r0 * np.float32(1e-15), None)]
    expect, where = {}, {}
    for i, (name, row, want) in enumerate(special):
        at = N - 1 - i // 2 if i % 2 == 0 else i // 2
        if 0 <= at < N and at not in where.values():
            ze[at] = row
            where[name] = at
            if want is not None:
                expect[at] = want
    return ze, expect, where


def nonfinite_rows():
    """An all-NaN row and a +-Inf row: every distance is NaN, the search keeps index 0 (as torch's max does)."""
    inf = np.array([np.inf, -np.inf, np.inf, np.inf, -np.inf, np.inf, -np.inf, -np.inf], np.float32)
    return np.full(DIM, np.nan, np.float32), inf


# ---- (c) fused forward -----------------------------------------------------------------------------------------------
FWD_D = (1, 15, 16, 17, 40, 96)
FWD_BT = ((1, 1), (1, 255), (1, 257), (3, 171))
FWD_CODES = (5, 1025, 8192)
MAX_SHARE = 0.01  # of a case's frames


def vq_params(D, n_codes, g):
    """Folded projections and a codebook for one FactorizedVectorQuantize (float32 tensors)."""
    return {"w_in": (torch.rand(DIM, D, generator=g) - 0.5) * (2.0 / D ** 0.5), "b_in": (torch.rand(DIM, generator=g) - 0.5) * 0.2,
            "cb": torch.randn(n_codes, DIM, generator=g), "w_out": torch.rand(D, DIM, generator=g) - 0.5,
            "b_out": (torch.rand(D, generator=g) - 0.5) * 0.2}


@functools.lru_cache(maxsize=None)
def fwd_case(D, B, T, n_codes):
    """Inputs and both restatements of one fused-forward case.  A seed is usable when the float32 and float64
    restatements disagree on at most MAX_SHARE of the frames, each disagreement at a float64 top-2 gap below GAP_TOL, and
    z_e / post are `usable`."""
    from helpers import GAP_TOL

    def make(seed):
        g = gen(seed)
        p = vq_params(D, n_codes, g)
        z = torch.randn(B, D, T, generator=g) * 2.0
        ze32, idx32, post32 = fvq(z, p, F32)
        ze64, idx64, post64 = fvq(z, p, F64)
        gap = search64(rows(ze64), p["cb"])[1].reshape(B, T)
        differ = (idx32 != idx64).numpy()
        if differ.sum() > MAX_SHARE * B * T or (differ.any() and gap[differ].max() >= GAP_TOL):
            return None
        if not usable(ze32, ze64) or not usable(post32, post_of(ze64, idx32, p, F64)):
            return None
        return dict(params=p, z=z, ze32=ze32, idx32=idx32, post32=post32, ze64=ze64, idx64=idx64, post64=post64, gap=gap,
                    differ=int(differ.sum()))

    return _first_usable(make, 40000 + 1000 * D + 10 * T + B + n_codes)


def fwd_cases():
    return [(D, B, T, n) for D in FWD_D for (B, T) in FWD_BT for n in FWD_CODES]


# ---- (d) vq2emb ------------------------------------------------------------------------------------------------------
EMB_D = (1, 31, 96)
EMB_N = (1, 257)
EMB_CODES = (5, 8192)


@functools.lru_cache(maxsize=None)
def emb_case(D, N, n_codes):
    """A 3-column index tensor (every code of a small codebook, the first and the last code of a large one), out_proj
    parameters, a known tensor to accumulate onto; usable for every column, with and without accumulation."""
    def make(seed):
        g = gen(seed)
        p = vq_params(D, n_codes, g)
        idx = torch.randint(0, n_codes, (N, 3), generator=g)
        flat = idx.reshape(-1)
        edge = torch.tensor([0, n_codes - 1] + list(range(min(n_codes, 5))))[: flat.numel()]
        flat[: edge.numel()] = edge
        base = torch.randn(N, D, generator=g)
        for col in range(3):
            for acc in (None, base):
                a = vq2emb(idx, col, p["cb"], p["w_out"], p["b_out"], acc, F32)
                b = vq2emb(idx, col, p["cb"], p["w_out"], p["b_out"], acc, F64)
                if not usable(a, b):
                    return None
        return dict(params=p, idx=idx, base=base)

    return _first_usable(make, 50000 + 1000 * D + N + n_codes)


def emb_cases():
    return [(D, N, n) for D in EMB_D for N in EMB_N for n in EMB_CODES]


# ---- (e) rvq_update --------------------------------------------------------------------------------------------------
RVQ_N = (1, 255, 257, 70000, 65536 * 256 + 257)  # the last: one element more than the launch's 65536 x 256 threads, + 256


RVQ_SIZES = (1025, 300, 8192)  # the three-layer ResidualVQ: a one-code last chunk, under one chunk, eight chunks


def rvq_case(n):
    rng = np.random.default_rng(6000 + n % 9973)
    r, o, q = (rng.standard_normal(n, dtype=np.float32) for _ in range(3))
    q[0] = -0.0  # 0. + (-0.) is +0.
    if n > 2:
        q[n // 2] = -0.0
        o[n // 2] = -0.0  # (-0.) + (-0.) stays -0. when not first
    return r, o, q


# ---- (f), (g) FSQ ----------------------------------------------------------------------------------------------------
FSQ_LEVELS = ((5,), (8, 5, 5), (4, 4, 4, 8), (8, 8, 8, 5, 5, 5), (3, 4, 3, 4, 3, 4, 3, 4))
FSQ_BT = ((1, 1), (2, 257))
FSQ_CODES_D = (1, 31, 33, 70)
FSQ_CODES_T = (1, 255, 257)


def fsq_widths(levels):
    return (len(levels) + 1, 33, 64)


def fsq_params(levels, D, g):
    d = len(levels)
    return {"w_in": (torch.rand(d, D, generator=g) - 0.5) * (4.0 / D ** 0.5), "b_in": (torch.rand(d, generator=g) - 0.5) * 0.2,
            "w_out": torch.rand(D, d, generator=g) - 0.5, "b_out": (torch.rand(D, generator=g) - 0.5) * 0.2}


@functools.lru_cache(maxsize=None)
def fsq_case(levels, D, B, T):
    """One FSQ forward case.  threshold = 4 x the float32 restatement's largest deviation from float64 in the bounded
    value; a seed is usable when at most MAX_SHARE of the frames have a margin at or under it, the restatements agree on
    every other frame, and post (on the float64 indices) is `usable`."""
    def make(seed):
        g = gen(seed)
        p = fsq_params(levels, D, g)
        z = torch.randn(B, D, T, generator=g) * 1.5
        args = (z, p["w_in"], p["b_in"], p["w_out"], p["b_out"], levels)
        post32, idx32, margin = fsq_forward(*args, F32)
        post64, idx64, _ = fsq_forward(*args, F64)
        dev = float((fsq_bounded(z, p["w_in"], p["b_in"], levels, F32).double()
                     - fsq_bounded(z, p["w_in"], p["b_in"], levels, F64)).abs().max())
        thr = 4.0 * dev
        excluded = (margin <= thr).numpy()
        if excluded.sum() > MAX_SHARE * B * T or bool((idx32 != idx64).numpy()[~excluded].any()):
            return None
        p32 = fsq_codes(idx64, levels, p["w_out"], p["b_out"], F32)
        if not usable(p32, post64) or excluded.all():
            return None
        return dict(params=p, z=z, post32=p32, post64=post64, idx64=idx64, idx32=idx32, margin=margin, threshold=thr,
                    excluded=excluded)

    return _first_usable(make, 70000 + 1000 * len(levels) + 10 * D + T + B)


def fsq_cases():
    return [(lv, D, B, T) for lv in FSQ_LEVELS for D in fsq_widths(lv) for (B, T) in FSQ_BT]


def fsq_code_indices(levels, T, bits):
    """(1, T) indices: every code of the grid (as far as T has room), negatives, values >= prod(levels), and for int64
    values beyond 2^31; the int32 list is the int64 one where int32 can hold it (else a value near its own limit)."""
    n = int(np.prod(levels))
    rng = np.random.default_rng(8000 + n + T)
    edge = [-1, n, -n, n + 1, 2 * n + 3, -n - 1, -12345, 2 ** 31 - 1, -2 ** 31, 0]
    far = [2 ** 31, 2 ** 31 + 5, -2 ** 31 - 7, 2 ** 40 + 11, -2 ** 45 - 3, 2 ** 62 + 1]
    vals = list(itertools.islice(itertools.chain(edge, far, range(n), rng.integers(-3 * n, 3 * n, T).tolist()), T))
    if T == 1:
        vals = [n + 1]
    a = np.array(vals, dtype=np.int64)[None]
    if bits == 32:
        fits = (a >= -2 ** 31) & (a < 2 ** 31)
        return np.where(fits, a, a % 2 ** 31).astype(np.int32), fits
    return a, np.ones_like(a, bool)


@functools.lru_cache(maxsize=None)
def fsq_codes_case(levels, D, T):
    def make(seed):
        g = gen(seed)
        p = fsq_params(levels, D, g)
        i64, _ = fsq_code_indices(levels, T, 64)
        if not usable(fsq_codes(i64, levels, p["w_out"], p["b_out"], F32), fsq_codes(i64, levels, p["w_out"], p["b_out"], F64)):
            return None
        return dict(params=p)

    return _first_usable(make, 90000 + 1000 * len(levels) + 10 * D + T)
