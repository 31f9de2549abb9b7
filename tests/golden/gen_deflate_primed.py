#!/usr/bin/env python3
"""Writes tests/golden/deflate_primed.json: (length, sha256[:16]) of what C zlib 1.2.11 produces
for every case of tests/primedcases.py -- the stream's ordinary wrapper header, then every piece
as a raw stream of its own, zlib.compressobj(level, DEFLATED, -15, 8, 0, zdict = the 32 KiB in
front of the piece), fed in 32,768-byte compress() calls, flush(Z_SYNC_FLUSH) behind every piece
but the last and flush() behind that, then the trailer over the whole input; a gzip header's OS
byte reads 0xff.  A deflate-raw case also lists the offsets behind its markers; a *long* case
also the single-stream size and the size flushed at the same positions.

zlib 1.2.11 is the yardstick, not the reference's TypeScript: the reference's stream layer never
passes a dictionary, Z_SYNC_FLUSH or a position.  Other zlib versions differ in deflate_fast /
deflate_slow details, so this script refuses to run on them.  For every case it
  - inflates the bytes back as ONE stream with zlib.decompress and compares with the input;
  - asserts zs_deflate_bound_flush;
  - asserts that the 32,768-byte feed and the whole-piece feed give the same bytes;
  - for a long case, asserts primed < flushed and prints single / primed / flushed;
and once, primedcases.cut_shown(): the cut cases hit the 16,383-symbol corner (how: its docstring).

    python tests/golden/gen_deflate_primed.py            # rewrite the file
    python tests/golden/gen_deflate_primed.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import primedcases as cases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    assert cases.cut_shown()
    out = {}
    for c in cases.all_cases():
        name, data, level, fmt, pos = c
        assert name not in out, name
        y = cases.yardstick(c)
        assert zlib.decompress(y, cases.WBITS[fmt]) == data, name
        assert len(y) <= cases.bound(len(data), fmt, len(pos)), name
        assert cases.compress(data, level, fmt, pos, feed=max(1, len(data))) == y, name
        out[name] = e = cases.entry(c)
        if name.startswith("long/"):
            single, flushed = e[3]
            assert e[0] < flushed, name  # (against the single stream it may fall on either side: the blocks are cut elsewhere)
            print("%s: single %d, primed %d (%+.3f %%), flushed %d (%+.3f %%)" % (
                name, single, e[0], 100.0 * (e[0] - single) / single, flushed, 100.0 * (flushed - single) / single))
    return out


def main():
    got = generate()
    if "--check" in sys.argv[1:]:
        with open(cases.GOLDEN) as f:
            want = json.load(f)
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        if bad:
            raise SystemExit("%d cases differ, first %s" % (len(bad), bad[0]))
        print("%d cases match" % len(got))
        return
    with open(cases.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in sorted(got.items())) + "\n}\n")
    print("wrote %d cases to %s" % (len(got), cases.GOLDEN))


if __name__ == "__main__":
    main()
