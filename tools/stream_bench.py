"""Causal streaming throughput on the GPU: a causal `default` BigCodec encoder (and decoder) fed chunk by chunk.

    python tools/stream_bench.py [--B 64] [--seconds 10] [--chunk 12000] [--prev] [--decode]

Prints audio-seconds per second of the stream (every chunk of a B-clip batch pushed back to back, HIP-synchronised
around the whole stream), ms per push and the number of kernel launches per push (rocprofv3 gives the names).
--graph replays one captured HIP graph per chunk (StreamGraph; status words read once at the end).
--prev times the round-4 first-session stream (tools/lab/streaming_prev.py: separate Snake launches, torch.cat
contexts, two-launch ResidualUnits) on the same models for an A/B.  Random weights, synthetic white noise.
--pool [--decode] [--pool-B 16 64] [--pool-frames 1 5] times a tick of B independent sessions through the session
pool (StreamPool), through one batched stream and through B single streams.
--pool --ragged [--decode] [--pool-B 16 64] times a tick in which every session has its own number of hops ready (1 to
5, drawn per tick with a fixed seed): one push with `hops` against one equal-length push per distinct length
(DESIGN.md §20).
--lookahead [--pool-B 1 16] [--la-hops 1 5 25] streams the NON-causal `default` encoder through LookaheadEncoder
(DESIGN.md §23): ms per push at each chunk length, and the clip-level cost of la.encode(x, chunk) over the
whole-sequence encoder(x) on the same --seconds clip.
--pool --lookahead [--decode] [--pool-B 16 64] [--ticks 40] times a tick of B NON-causal `default` sessions that open
at different ticks and deliver 1 to 5 hops each: one LookaheadPool push against one B = 1 look-ahead stream per session
(DESIGN.md §24).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools", "lab"))

import torch  # noqa: E402

from audiotokenization_amd import config, synth  # noqa: E402
from audiotokenization_amd.codec import BigCodecDecoder, BigCodecEncoder  # noqa: E402
from audiotokenization_amd.extract import synth_batch  # noqa: E402


def build_model_pair(name, device, **ov):
    """Encoder / decoder of preset `name` with synthetic weights (bench.py's build_model)."""
    cfg = config.preset(name, **ov)
    enc = BigCodecEncoder(**config.encoder_kwargs(cfg.model.codec_encoder))
    dec = BigCodecDecoder(**config.decoder_kwargs(cfg.model.codec_decoder))
    for m, prefix in ((enc, "encoder."), (dec, "decoder.")):
        syn = synth.synth_state_dict({prefix + k: v for k, v in m.state_dict().items()})
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in syn.items()}, strict=True)
    return enc.eval().to(device), dec.eval().to(device)


def pool_leg(a, dev, enc, dec):
    """--pool: B live sessions, one chunk each per tick, three ways in one run (alternating, best of --reps after a
    warm-up round): (a) StreamPool.push, (b) one StreamingEncoder / StreamingDecoder of batch B (the lower bound: the
    same kernels without the indirection, but its sessions must start and end together), (c) B separate B = 1 streams
    pushed one after another (what independent sessions cost without the pool).  One JSON line per (B, frames)."""
    import json

    from audiotokenization_amd import streaming as S

    model, hop = (dec, 1) if a.decode else (enc, int(enc.hop_length))
    stream_cls = S.StreamingDecoder if a.decode else S.StreamingEncoder
    only = a.pool_only.split(",") if a.pool_only else ["pool", "batch", "singles"]
    for B in a.pool_B:
        for frames in a.pool_frames:
            n = frames * hop
            x = synth_batch(B, a.ticks * frames * int(enc.hop_length), 0, dev)
            with torch.no_grad():
                data = dec(enc(x), vq=True)[0] if a.decode else x
                pool = S.StreamPool(model, B)
                sids = [pool.open() for _ in range(B)]
                batch = stream_cls(model)
                singles = [stream_cls(model) for _ in range(B)]
                legs = {
                    "pool": lambda c: pool.push(sids, c),
                    "batch": lambda c: batch.push(c),
                    "singles": lambda c: [s.push(c[b:b + 1]) for b, s in enumerate(singles)],
                }
                best = {}
                for rep in range(a.reps + 1):
                    for name in only:
                        if name == "setup":  # nothing but the set-up: what a kernel trace of one leg subtracts
                            continue
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for t in range(a.ticks):
                            legs[name](data[..., t * n:(t + 1) * n])
                        torch.cuda.synchronize()
                        dt = 1e3 * (time.perf_counter() - t0) / a.ticks
                        if rep:  # the first round warms the weight caches and sizes the state
                            best[name] = min(best.get(name, dt), dt)
            print(json.dumps(dict(leg="pool", what="decode" if a.decode else "encode", B=B, frames=frames, ticks=a.ticks,
                                  ms_per_tick={k: round(v, 3) for k, v in best.items()},
                                  state_bytes_per_session=pool.state_bytes() // B)), flush=True)


def ragged_leg(a, dev, enc, dec):
    """--pool --ragged: B live sessions, each with 1 ... 5 hops ready per tick (uniform, seeded), two ways in one run
    (alternating, best of --reps after a warm-up round): (a) one push with `hops` over the batch padded to the tick's
    longest entry, (b) what a service did before: the sessions grouped by length, one equal-length push per group.
    Each leg has its own pool of B sessions and walks the same per-session streams; the padded and the grouped
    batches are assembled before the timed window (both legs get ready-made tensors).  One JSON line per B."""
    import json
    import random

    from audiotokenization_amd import streaming as S

    model, unit = (dec, 1) if a.decode else (enc, int(enc.hop_length))
    for B in a.pool_B:
        rng = random.Random(a.seed)
        draws = [[rng.randint(1, 5) for _ in range(B)] for _ in range(a.ticks)]
        total = max(sum(d[b] for d in draws) for b in range(B))
        x = synth_batch(B, total * int(enc.hop_length), 0, dev)
        with torch.no_grad():
            data = dec(enc(x), vq=True)[0] if a.decode else x
            pools = {name: S.StreamPool(model, B) for name in ("ragged", "grouped")}
            sids = {name: [p.open() for _ in range(B)] for name, p in pools.items()}
            pos, padded, grouped = [0] * B, [], []
            for hops in draws:
                n_hops = max(hops)
                xt = torch.zeros(B, data.shape[1], n_hops * unit, device=dev)
                for b, h in enumerate(hops):
                    xt[b, :, :h * unit] = data[b, :, pos[b]:pos[b] + h * unit]
                padded.append((xt, hops))
                groups = []
                for h in sorted(set(hops)):
                    members = [b for b in range(B) if hops[b] == h]
                    groups.append((members, torch.stack([data[b, :, pos[b]:pos[b] + h * unit] for b in members])))
                grouped.append(groups)
                pos = [p + h * unit for p, h in zip(pos, hops)]

            def run_ragged():
                pool, ids = pools["ragged"], sids["ragged"]
                for xt, hops in padded:
                    pool.push(ids, xt, hops=hops)

            def run_grouped():
                pool, ids = pools["grouped"], sids["grouped"]
                for groups in grouped:
                    for members, xg in groups:
                        pool.push([ids[b] for b in members], xg)

            best = {}
            for rep in range(a.reps + 1):
                for name, leg in (("ragged", run_ragged), ("grouped", run_grouped)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg()
                    torch.cuda.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0) / a.ticks
                    if rep:  # the first round warms the weight caches and sizes the state
                        best[name] = min(best.get(name, dt), dt)
        print(json.dumps(dict(leg="ragged", what="decode" if a.decode else "encode", B=B, ticks=a.ticks, seed=a.seed,
                              pushes_per_tick=dict(ragged=1.0, grouped=round(sum(len(g) for g in grouped) / a.ticks, 2)),
                              ms_per_tick={k: round(v, 3) for k, v in best.items()},
                              grouped_over_ragged=round(best["grouped"] / best["ragged"], 2))), flush=True)


def lookahead_leg(a, dev):
    """--lookahead: the non-causal `default` encoder, current precision (x6 unless BIGCODEC_PRECISION says otherwise).
    Per (B, hops per push): la.encode(x, chunk) and encoder(x) on the same clip, alternating, one untimed pass of each
    first (it warms every window shape of the transient as well as the steady ones), then --reps timed passes of each,
    HIP-synchronised around a pass; medians.  ms per push = the stream's clip time over its pushes (the finish counts
    as one).  One JSON line per (B, hops)."""
    import json
    import statistics

    from audiotokenization_amd import _lib as L
    from audiotokenization_amd import streaming as S

    enc, _ = build_model_pair("default", device=dev)
    hop = int(enc.hop_length)
    n = int(a.seconds * 24000) // hop * hop
    la = S.LookaheadEncoder(enc)
    for B in a.pool_B:
        x = synth_batch(B, n, 0, dev)
        for hops in a.la_hops:
            chunk = hops * hop
            times = {"stream": [], "whole": []}
            with torch.no_grad():
                equal = bool(torch.equal(la.encode(x, chunk), enc(x)))
                for _ in range(a.reps):
                    for name, fn in (("stream", lambda: la.encode(x, chunk)), ("whole", lambda: enc(x))):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[name].append(1e3 * (time.perf_counter() - t0))
            med = {k: statistics.median(v) for k, v in times.items()}
            pushes = n // chunk + 1
            print(json.dumps(dict(leg="lookahead", model="default", precision=L.precision_name(), B=B, hops=hops,
                                  seconds=n / 24000, lookahead_samples=la.lookahead, pushes=pushes,
                                  ms_per_push=round(med["stream"] / pushes, 4), stream_ms=round(med["stream"], 2),
                                  whole_ms=round(med["whole"], 2), ratio=round(med["stream"] / med["whole"], 3),
                                  stream_ms_all=[round(t, 2) for t in times["stream"]],
                                  whole_ms_all=[round(t, 2) for t in times["whole"]], equal=equal)), flush=True)


def lookahead_pool_leg(a, dev):
    """--pool --lookahead [--decode]: B sessions of the non-causal `default` model, session i opened at tick i mod 8 (so
    the pool always holds sessions in their transient), each drawing 1 ... 5 hops per tick (seeded), for --ticks ticks,
    two ways in one run (alternating, best of --reps after a warm-up round): (a) ONE LookaheadPool push per tick, (b)
    one B = 1 LookaheadEncoder / LookaheadDecoder per session, pushed one after another (what a service over a
    non-causal checkpoint did before).  Both walk the same per-session streams; the padded batches and the B = 1
    chunks are assembled before the timed window.  One JSON line per B."""
    import json
    import random

    from audiotokenization_amd import _lib as L
    from audiotokenization_amd import streaming as S

    enc, dec = build_model_pair("default", device=dev)
    model, unit = (dec, 1) if a.decode else (enc, int(enc.hop_length))
    stream_cls = S.LookaheadDecoder if a.decode else S.LookaheadEncoder
    for B in a.pool_B:
        rng = random.Random(a.seed)
        draws = [[rng.randint(1, 5) if t >= b % 8 else 0 for b in range(B)] for t in range(a.ticks)]
        total = max(sum(d[b] for d in draws) for b in range(B))
        x = synth_batch(B, total * int(enc.hop_length), 0, dev)
        with torch.no_grad():
            data = dec(enc(x), vq=True)[0] if a.decode else x
            pos, padded, chunks = [0] * B, [], []
            for hops in draws:
                members = [b for b in range(B) if hops[b]]
                xt = torch.zeros(len(members), data.shape[1], max(hops) * unit, device=dev)
                for i, b in enumerate(members):
                    xt[i, :, :hops[b] * unit] = data[b, :, pos[b]:pos[b] + hops[b] * unit]
                padded.append((members, xt, [hops[b] for b in members]))
                chunks.append([(b, data[b:b + 1, :, pos[b]:pos[b] + hops[b] * unit].contiguous()) for b in members])
                pos = [p + h * unit for p, h in zip(pos, hops)]
            pool = S.LookaheadPool(model, B)
            singles = [stream_cls(model) for _ in range(B)]
            emitted = {}

            def run_pool():
                sids, out = {}, 0
                for members, xt, hops in padded:
                    for b in members:
                        if b not in sids:
                            sids[b] = pool.open()
                    out += sum(pool.push([sids[b] for b in members], xt, hops=hops)[1])
                for s in sids.values():
                    pool.close(s)
                emitted["pool"] = out

            def run_singles():
                out = 0
                for s in singles:
                    s.reset()
                for tick in chunks:
                    for b, c in tick:
                        out += singles[b].push(c).shape[-1]
                emitted["singles"] = out

            best = {}
            for rep in range(a.reps + 1):
                for name, leg in (("pool", run_pool), ("singles", run_singles)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg()
                    torch.cuda.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0) / a.ticks
                    if rep:  # the first round warms the weight caches, every window shape and sizes the state
                        best[name] = min(best.get(name, dt), dt)
            assert emitted["pool"] == emitted["singles"], emitted  # both arms handed out the same columns
        print(json.dumps(dict(leg="lookahead_pool", model="default", precision=L.precision_name(),
                              what="decode" if a.decode else "encode", B=B, ticks=a.ticks, seed=a.seed,
                              pushes_per_tick=dict(pool=1.0, singles=round(sum(len(c) for c in chunks) / a.ticks, 2)),
                              columns_out=emitted["pool"], ms_per_tick={k: round(v, 3) for k, v in best.items()},
                              singles_over_pool=round(best["singles"] / best["pool"], 2),
                              state_bytes_per_session=pool.state_bytes() // B)), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lookahead", action="store_true", help="LookaheadEncoder on the non-causal default model")
    p.add_argument("--la-hops", type=int, nargs="+", default=[1, 5, 25], help="--lookahead: hops per push")
    p.add_argument("--pool", action="store_true", help="session-pool push vs one batched stream vs B single streams")
    p.add_argument("--pool-B", type=int, nargs="+", default=[16, 64])
    p.add_argument("--pool-frames", type=int, nargs="+", default=[1, 5], help="frames (hops) per session and tick")
    p.add_argument("--pool-only", default="", help="comma list of pool,batch,singles,setup (a kernel trace of one of them)")
    p.add_argument("--ragged", action="store_true", help="with --pool: one push with hops vs one push per distinct length")
    p.add_argument("--seed", type=int, default=0, help="--ragged: seed of the hops drawn per session and tick")
    p.add_argument("--ticks", type=int, default=10)
    p.add_argument("--B", type=int, default=64)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--chunk", type=int, default=12000, help="samples per push (encode) / x hop (decode)")
    p.add_argument("--prev", action="store_true")
    p.add_argument("--decode", action="store_true")
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--graph", action="store_true", help="push through a StreamGraph (one HIP-graph replay per chunk)")
    a = p.parse_args()
    if a.prev:
        import streaming_prev as S
    else:
        from audiotokenization_amd import streaming as S
    dev = torch.device("cuda:0")
    if a.lookahead:
        return (lookahead_pool_leg if a.pool else lookahead_leg)(a, dev)
    enc, dec = build_model_pair("default", device=dev, causal=True)
    if a.pool:
        return (ragged_leg if a.ragged else pool_leg)(a, dev, enc, dec)
    n = int(a.seconds * 24000) // 200 * 200
    x = synth_batch(a.B, n, 0, dev)
    with torch.no_grad():
        if a.decode:
            z = dec(enc(x), vq=True)[0]
            s = S.StreamingDecoder(dec)
            step = a.chunk // 200
            data, width = z, step
        else:
            s = S.StreamingEncoder(enc)
            data, width = x, a.chunk
        best = None
        g = s.graph(data[..., :width]) if a.graph else None
        if g is not None and data.shape[-1] % width:
            raise SystemExit("--graph needs the stream length to be a multiple of the chunk")
        for _ in range(a.reps + 1):
            s.reset() if g is None else g.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pushes = 0
            for i in range(0, data.shape[-1], width):
                if g is not None:
                    g.push(data[..., i:i + width], check=False)
                else:
                    s.push(data[..., i:i + width])
                pushes += 1
            if g is not None:
                g.check()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    what = "decode" if a.decode else "encode"
    mode = "prev" if a.prev else ("graph" if a.graph else "current")
    print(f"stream {what} ({mode}): B {a.B} x {n / 24000:.1f} s, chunk {a.chunk} samples, "
          f"{pushes} pushes: {a.B * n / 24000 / best:.1f} audio-s/s, {1e3 * best / pushes:.2f} ms per push")


if __name__ == "__main__":
    main()
