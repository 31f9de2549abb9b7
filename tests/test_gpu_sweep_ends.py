"""GPU parity of zs_k_sweep's groups in which a lane's chain ends (deflate_sweep.hip,
SwWave::ends, remask, open8; the rule is csrc/zs_sweep_ends.h): the group's unmasked maximum is
kept unless a dead step -- a member of the neighbouring bucket, or an occurrence more than
MAX_DIST back -- would win or is long, and then the wave masks its scores step by step.

The streams of tests/sweependscases.py put such dead steps where they matter: full signature
matches in the bucket before the lane's own (dead winner and dead long), five-byte ones against
live steps of three and four, a window death behind step 8 and inside steps 1..8, head
candidates at exactly MAX_DIST and one past it, and buckets that start mid-chunk so that the
lanes die eight per group.  tests/test_sweep_ends_model.py asserts that the cases occur; here
the output must be the oracle's bytes and the sweep's match table the chain walk's (option
match_sweep = 0) at every position, at levels 5, 6, 7 and 9 (both ring forms), in both signature
forms."""
import pytest

import oracle
import sweependscases


@pytest.fixture(scope="module")
def streams():
    return sweependscases.streams()


@pytest.fixture(scope="module")
def wanted(streams):
    """The oracle's output per (stream, level), computed once."""
    return {(k, lv): oracle.compress(d, lv, "deflate-raw")[1] for k, d in streams.items() for lv in (5, 6, 7, 9)}


@pytest.mark.gpu
@pytest.mark.parametrize("level", [5, 6, 7, 9])
def test_sweep_ends_bytes_and_match_table(engine, streams, wanted, level):
    names = sorted(streams)
    inputs = [streams[k] for k in names]
    tables, outs = [], []
    try:
        for sweep in (1, 0):
            engine.set_option("match_sweep", sweep)
            outs.append(engine.compress_batch_raw(inputs, "deflate-raw", level))
            tables.append([engine.debug_fetch(1, i, 8 * len(d)) for i, d in enumerate(inputs)])
    finally:
        engine.set_option("match_sweep", 1)
    for i, k in enumerate(names):
        assert outs[0][i] == (1, wanted[(k, level)]), k
        assert len(tables[0][i]) == 8 * len(inputs[i]), k
        assert tables[0][i] == tables[1][i], k
        assert outs[1][i] == outs[0][i], k
