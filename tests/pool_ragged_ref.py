"""The ragged pool schedule shared by tests/test_gpu_stream_pool_ragged.py and the child process it
starts on the bounds-checked debug build: five sessions on three slots whose pushes hold one to three sessions with a
different number of hops each, and the runner that feeds it to a StreamPool or a PoolGraph."""
import torch

from audiotokenization_amd import synth

HOPS = {"A": 12, "B": 7, "C": 9, "D": 5, "E": 6}  # session lengths in hops (frames), as in test_gpu_stream_pool.py
CAPACITY = 3
# (sessions opened before the push, the push's sessions in order, hops per session in this push, sessions closed after)
SCHEDULE = [
    ("A", "A", (2,), ""),
    ("B", "BA", (3, 1), ""),         # one hop under n_hops = 3
    ("C", "ABC", (2, 1, 3), ""),
    ("", "CA", (1, 2), ""),          # B sits this tick out
    ("", "BCA", (3, 2, 1), "B"),     # B ends; D gets its slot
    ("D", "DAC", (1, 3, 2), ""),
    ("", "AD", (1, 2), "A"),         # A ends; E gets its slot
    ("E", "CE", (1, 3), "C"),
    ("", "ED", (3, 2), "ED"),
]
REUSE = {"D": "B", "E": "A"}  # who must get whose session id
N_MAX = 3  # the most hops an entry of the schedule delivers


def clip(s, hop, dev):
    n = HOPS[s] * hop
    return torch.from_numpy(synth.synth_clips(1, n, clip0=50 + ord(s))).unsqueeze(1).to(dev)


def run_schedule(pool, inputs, unit, out_unit, push=None, pad_to=None, tail=float("nan")):
    """SCHEDULE on `pool`: inputs[s] (1, C, HOPS[s] * unit) is session s's whole input (float, or integer codes laid
    out (1, Nq, frames)); every push is a padded batch of n_hops = max(hops) (or pad_to) hops whose row i holds
    hops[i] hops of its session, left-aligned, and `tail` (NaN; -1 for codes: an index the decoder turns into NaN)
    behind them.  `push(sids, x, hops)`: pool.push unless given (the token entry, a graph).  Checks the padded shape,
    the exactly-zero output tails and pool.samples after every push; returns each session's concatenated valid
    output."""
    push = push or pool.push
    sid, pos, out, closed_id = {}, {s: 0 for s in HOPS}, {s: [] for s in HOPS}, {}
    sizes = set()
    for opened, members, hops, closed in SCHEDULE:
        for s in opened:
            sid[s] = pool.open()
            if s in REUSE:
                assert sid[s] == closed_id[REUSE[s]], (s, sid[s], closed_id)
        assert len(members) == len(hops) and len(pool.live()) <= CAPACITY
        n_hops = pad_to or max(hops)
        first = inputs[members[0]]
        x = torch.full((len(members), first.shape[1], n_hops * unit), tail, dtype=first.dtype, device=first.device)
        for i, (s, h) in enumerate(zip(members, hops)):
            x[i, :, :h * unit] = inputs[s][0, :, pos[s]:pos[s] + h * unit]
        y = push([sid[s] for s in members], x, list(hops))
        assert y.shape[0] == len(members) and y.shape[2] == n_hops * out_unit, (y.shape, members, hops)
        for i, (s, h) in enumerate(zip(members, hops)):
            out[s].append(y[i:i + 1, :, :h * out_unit].clone())
            rest = y[i, :, h * out_unit:]
            assert not rest.numel() or int(rest.contiguous().view(torch.int32).abs().max()) == 0, \
                f"session {s}: the output past its {h} hops is not +0.0"
            pos[s] += h * unit
            assert pool.samples(sid[s]) == pos[s] // unit * pool.hop, (s, pool.samples(sid[s]), pos[s])
        sizes.add(len(members))
        for s in closed:
            assert pos[s] == inputs[s].shape[-1], f"session {s} closed before its input ended"
            pool.close(sid[s])
            closed_id[s] = sid[s]
    assert sizes == {1, 2, 3} and pool.live() == []
    return {s: torch.cat(v, dim=2) for s, v in out.items()}
