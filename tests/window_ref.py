"""The streaming window of csrc/elementwise.hip (window_kernel) in plain torch indexing, on the CPU in float32: the one
formula behind the five bc_stream_window* entry points, with the general per-entry arguments.  For each entry b and
every channel

    win[j] = j < ci ? (src >= 0 ? carry[src][j] : 0) : j < ci + n ? xa[xo + j - ci] : 0      (j < W)
    out[dst][i] = win[keep + i]   for i < co                                                  (dst >= 0)

xa is x AFTER the activation (the caller runs the product's own snake op over x, so values move by copies alone and
bits must match).  Only copies touch the data, so NaN payloads survive and bit patterns can be compared."""
import torch


def window_ref(xa, carry, src, out, dst, ci, n, xo, keep, co, W):
    """(win (B, C, W), out after the stores).  xa (B, C, xn); carry (rows, C, pitch) or None; out (rows', C, pitch') is
    not modified, its copy is; src, dst, ci, n, xo, keep, co: one int per entry."""
    B, C = xa.shape[:2]
    win = torch.zeros(B, C, W, dtype=torch.float32)
    out = out.clone()
    for b in range(B):
        assert 0 <= ci[b] and 0 <= n[b] and ci[b] + n[b] <= W and 0 <= xo[b] and xo[b] + n[b] <= xa.shape[2]
        if src[b] >= 0 and ci[b]:
            win[b, :, :ci[b]] = carry[src[b], :, :ci[b]]
        if n[b]:
            win[b, :, ci[b]:ci[b] + n[b]] = xa[b, :, xo[b]:xo[b] + n[b]]
        if dst[b] >= 0 and co[b]:
            assert 0 <= keep[b] and keep[b] + co[b] <= ci[b] + n[b]  # a carry never holds one of the zeros behind
            out[dst[b], :, :co[b]] = win[b, :, keep[b]:keep[b] + co[b]]
    return win, out


def bits(t):
    """The bit patterns of a float32 tensor (NaN payloads included), on the CPU."""
    return t.detach().cpu().contiguous().view(torch.int32)


def window_lens(ctx, x, L):
    """bc_stream_window_slots_lens for one row: (win, next context) from ctx (P,), the padded chunk x (n,) and L."""
    P, n = ctx.numel(), x.numel()
    win, nxt = window_ref(x.view(1, 1, n), ctx.view(1, 1, P), [0], torch.zeros(1, 1, P), [0], [P], [L], [0], [L], [P],
                          P + n)
    return win[0, 0], nxt[0, 0]


def window_equal(ctx, x):
    """bc_stream_window_slots for one row: win = [ctx | x], next context = win[n:]."""
    return window_lens(ctx, x, x.numel())
