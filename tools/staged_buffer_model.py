"""A CPU model of ONE wave of the one-lane search kernel's STAGED RESULTS (csrc/search_solo.h): how many results leave
unstaged, by the rule that gives a group of 8 queries its LDS buffer -- `g mod RES_BUFS` (before) or any free buffer.

    python tools/staged_buffer_model.py [--waves N] [--seed S]

The wave is the kernel's loop, pass by pass: a lane whose search has ended takes up the query it holds in reserve; the
lanes without a reserve draw the chunk's next queries in lane order; the groups that begin among the draws claim their
buffers; every running search then spends the pass, and one that ends puts its result into its group's buffer (freed
by the eighth) or stores it itself.  A search lasts `long` passes (it occurs in the shard) or 2..5 (it does not),
alternating, as bench.py's and the probes' batches interleave them.  Chunks of `qchunk` queries come from a counter
all waves share: at the headline (qchunk 1024) a wave's 128 groups per chunk are consecutive numbers; on the test's
two-shard set (qchunk 64, about 293 draws per wave) a wave's chunks are 8 groups each, from anywhere in the batch.

These are model numbers (DESIGN section 9 sets them beside the counter's); prints one JSON line."""
import json
import random
import sys

RES_BUFS = 28


def wave(rng, qchunk, chunks, long_passes, any_free, draws_limit=None):
    """one wave; returns (results, unstaged, sum over passes of open groups, passes)"""
    running = [None] * 64   # (group, passes left) per lane
    reserve = [None] * 64   # (group, length)
    left = [0] * RES_BUFS      # its results still out
    buf_of = {}                # open group -> buffer or None (unstaged)
    nxt = end = 0
    chunk_no = 0
    drawn = results = unstaged = open_sum = passes = 0
    while True:
        for lane in range(64):  # take-up
            if running[lane] is None and reserve[lane] is not None:
                running[lane], reserve[lane] = reserve[lane], None
        if nxt >= end and chunk_no < chunks:  # the next chunk: anywhere in the batch
            nxt = rng.randrange(1 << 20) * qchunk
            end = nxt + qchunk
            chunk_no += 1
        for lane in range(64):  # draw
            if reserve[lane] is not None or nxt >= end or (draws_limit is not None and drawn >= draws_limit):
                continue
            q, g = nxt, nxt >> 3
            nxt += 1
            drawn += 1
            if q & 7 == 0:  # the group begins: its claim
                if any_free:
                    free = [b for b in range(RES_BUFS) if left[b] == 0]
                    b = free[0] if free else None
                else:
                    b = g % RES_BUFS if left[g % RES_BUFS] == 0 else None
                buf_of[g] = b
                if b is not None:
                    left[b] = 8
            length = long_passes if q & 1 == 0 else rng.randint(2, 5)  # (present and random queries alternate in the batch)
            reserve[lane] = (g, length)
        if all(r is None for r in running) and all(r is None for r in reserve):
            if chunk_no >= chunks or (draws_limit is not None and drawn >= draws_limit):
                break
            continue
        for lane in range(64):  # the pass
            if running[lane] is None:
                continue
            g, n = running[lane]
            if n > 1:
                running[lane] = (g, n - 1)
                continue
            running[lane] = None
            results += 1
            b = buf_of[g]
            if b is None:
                unstaged += 1
            else:
                left[b] -= 1
        open_sum += sum(1 for x in left if x)
        passes += 1
    return results, unstaged, open_sum, passes


def shape(name, seed, waves, **kw):
    out = {}
    for rule, any_free in (("g_mod_28", False), ("any_free_buffer", True)):
        rng = random.Random(seed)
        r = u = o = p = 0
        for _ in range(waves):
            a, b, c, d = wave(rng, any_free=any_free, **kw)
            r, u, o, p = r + a, u + b, o + c, p + d
        out[rule] = {"results": r, "unstaged": u, "unstaged_share": round(u / r, 4), "groups_open_on_average": round(o / p, 1)}
    return {name: out}


def main(argv):
    waves = int(argv[argv.index("--waves") + 1]) if "--waves" in argv else 8
    seed = int(argv[argv.index("--seed") + 1]) if "--seed" in argv else 1
    report = {"res_bufs": RES_BUFS, "waves_per_shape": waves}
    report |= shape("headline_qchunk_1024_16_pass_searches", seed, waves, qchunk=1024, chunks=4, long_passes=16)
    report |= shape("test_set_qchunk_64_22_pass_searches_293_draws", seed, 16 * waves, qchunk=64, chunks=5, long_passes=22, draws_limit=293)
    print(json.dumps(report))


if __name__ == "__main__":
    main(sys.argv[1:])
