"""GPU parity of zs_k_sweep where its chunk and run boundaries fall: levels 4..6
sweep with the persistent per-wave ring (runs of consecutive chunks,
deflate_sweep.hip sw_body<., ., true>), levels 7 and 9 with the per-chunk ring.
Both must give the chain walk's match table (option match_sweep = 0) -- both
budgets and the slide-NIL flag, at every position -- and the oracle's bytes,
whichever wave gets which run."""
import hashlib

import pytest

import corpus
import oracle

pytestmark = pytest.mark.gpu

# members m = n - 2: 1, 64, 65, 128, 129, 192, 193, 512, 513, 576, 577, ... (chunks of 64, ring blocks, run ends)
LENGTHS = [3, 66, 67, 130, 131, 194, 195, 514, 515, 578, 579, 1026, 4099, 32506 + 70, 65536, 65537]


def _noise7(seed, n):
    return bytes(x & 0x7F for x in corpus.rand(seed, n))


KINDS = {
    "zeros": lambda seed, n: bytes(n),  # one bucket, every chain at full budget, the MAX_DIST cut
    "abcd": lambda seed, n: bytes(0x41 + (x & 3) for x in corpus.rand(seed, n)),  # deep 7-bit chains
    "text": corpus.text,
    "rand": corpus.rand,  # many buckets per chunk, chains ending in the first steps
    "mixed": corpus.mixed,  # 8-bit bytes: the 11-byte signature form
    "noise7+text": lambda seed, n: _noise7(seed, n * 3 // 10) + corpus.text(seed + 1, n - n * 3 // 10),
}
# streams over 65,537 bytes are swept in windows: chunks of look-back members only have no own lane
WINDOWED = [("text", 65538), ("text", 98303), ("zeros", 130836), ("mixed", 200001)]


@pytest.fixture(scope="module")
def inputs():
    out = []
    for ki, kind in enumerate(sorted(KINDS)):
        for n in LENGTHS:
            d = KINDS[kind](9000 + 100 * ki + (n & 63), n)
            assert len(d) == n
            out.append(d)
    for i, (kind, n) in enumerate(WINDOWED):
        out.append(KINDS[kind](9900 + i, n))
    return out


@pytest.mark.parametrize("level", [4, 5, 6, 7, 9])
def test_sweep_runs_match_table_equals_chain_walk(engine, inputs, level):
    tables, outs = [], []
    try:
        for sweep in (1, 0):
            engine.set_option("match_sweep", sweep)
            outs.append(engine.compress_batch_raw(inputs, "deflate-raw", level))
            tables.append([engine.debug_fetch(1, i, 8 * len(d)) for i, d in enumerate(inputs)])
    finally:
        engine.set_option("match_sweep", 1)
    for i, d in enumerate(inputs):
        assert len(tables[0][i]) == 8 * len(d), (i, len(d))
        assert tables[0][i] == tables[1][i], (i, len(d))
        want = oracle.compress(d, level, "deflate-raw")[1]
        assert outs[0][i] == outs[1][i] and outs[0][i] == (1, want), (i, len(d))


def test_sweep_runs_are_deterministic(engine):
    """The same 64-stream batch three times: which wave claims which run varies, the tables do not."""
    batch = [KINDS[sorted(KINDS)[i % len(KINDS)]](9500 + i, 65536 - 517 * (i % 7)) for i in range(64)]
    digests = []
    for _ in range(3):
        res = engine.compress_batch_raw(batch, "deflate-raw", 6)
        assert all(st == 1 for st, _ in res)
        h = hashlib.sha256()
        for i, d in enumerate(batch):
            t = engine.debug_fetch(1, i, 8 * len(d))
            assert len(t) == 8 * len(d)
            h.update(t)
        for _, out in res:
            h.update(out)
        digests.append(h.hexdigest())
    assert digests[0] == digests[1] == digests[2]
