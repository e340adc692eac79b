"""The look-ahead pool schedule shared by tests/test_lookahead_pool_host.py (a float64 toy stack),
tests/test_gpu_lookahead_pool.py (real models) and the child process the latter starts on the bounds-checked build."""
import torch

CAPACITY = 3
# per tick: {session: hops} served by ONE batched push ((hops, "F"): that entry flushes in the same push), then
# {session: remaining input columns or None} served by one finish call.  Five sessions of different lengths on three
# slots: B opens while A is past its first pushes and C while both are, so a push holds sessions in their transient
# next to steady ones; A, B and C sit ticks out; D and E reuse the slots A and C freed; hops are drawn from {1, 2, 3}.
TICKS = [
    (dict(A=2), {}),
    (dict(B=3, A=1), {}),
    (dict(B=1, C=2), {}),
    (dict(C=1, A=3, B=2), {}),
    (dict(A=2, C=3), {}),
    (dict(B=2, A=(3, "F"), C=3), {}),  # A flushes in the push that serves B and C
    (dict(D=1, B=1), {}),  # D: fresh, in A's slot
    (dict(D=2, B=3), dict(C=None)),  # C: finish() without input
    (dict(E=3, D=3), dict(B=3)),  # E: fresh, in C's slot; B: a remainder of 3 columns
    (dict(D=2, E=3), {}),
    (dict(E=1, D=2), {}),
    ({}, dict(E=0, D=6)),  # one finish for both: E delivers nothing more, D a remainder of 6
]
ORDER = "ABCDE"
REUSE = {"D": "A", "E": "C"}


def totals(unit):
    """Input columns per session for `unit` columns per hop."""
    T = {}
    for pushes, fins in TICKS:
        for s, h in pushes.items():
            T[s] = T.get(s, 0) + (h[0] if isinstance(h, tuple) else h) * unit
        for s, rem in fins.items():
            T[s] += rem or 0
    assert list(T) == list(ORDER)
    return T


def run_schedule(data, unit, open_, push, finish, tail=float("nan")):
    """TICKS on a pool: data[s] (1, C, totals(unit)[s]) is session s's whole input.  Every call gets a padded batch
    whose row i holds its session's columns, left-aligned, and `tail` behind them (NaN; -1 for codes).
    push(sids, x, hops, flags) and finish(sids, x or None, lens or None) return (y, counts).  Checks the exactly-zero
    output tails; returns (outs[s]: the claimed columns per call, chunks[s]: the input columns per call, sid)."""
    sid, pos = {}, {}
    outs, chunks = {s: [] for s in data}, {s: [] for s in data}
    first = data[ORDER[0]]

    def batch(names, lens):
        x = torch.full((len(names), first.shape[1], max(lens)), tail, dtype=first.dtype, device=first.device)
        for i, (s, n) in enumerate(zip(names, lens)):
            x[i, :, :n] = data[s][0, :, pos[s]:pos[s] + n]
            pos[s] += n
            chunks[s].append(n)
        return x

    def collect(names, y, counts):
        assert y.shape[0] == len(names) and y.shape[2] == max(counts), (y.shape, counts)
        for i, s in enumerate(names):
            rest = y[i, :, counts[i]:]
            assert not rest.numel() or float(rest.abs().max()) == 0, f"session {s}: the output past its columns is not zero"
            outs[s].append(y[i:i + 1, :, :counts[i]].clone())

    for pushes, fins in TICKS:
        if pushes:
            names = list(pushes)
            for s in names:
                if s not in sid:
                    sid[s], pos[s] = open_(), 0
                    assert s not in REUSE or sid[s] == sid[REUSE[s]], (s, sid)
            hops = [h[0] if isinstance(h, tuple) else h for h in pushes.values()]
            flags = [isinstance(h, tuple) for h in pushes.values()]
            x = batch(names, [h * unit for h in hops])
            collect(names, *push([sid[s] for s in names], x, hops, flags))
        if fins:
            names = list(fins)
            if all(v is None for v in fins.values()):
                for s in names:
                    chunks[s].append(0)
                collect(names, *finish([sid[s] for s in names], None, None))
            else:
                lens = [v or 0 for v in fins.values()]
                collect(names, *finish([sid[s] for s in names], batch(names, lens), lens))
    assert all(pos[s] == data[s].shape[-1] for s in data)
    assert len(set(sid.values())) == CAPACITY
    return outs, chunks, sid
