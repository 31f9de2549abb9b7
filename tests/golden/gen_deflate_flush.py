#!/usr/bin/env python3
"""Writes tests/golden/deflate_flush.json: (length, sha256[:16]) of what C zlib 1.2.11 produces
for every case of tests/flushcases.py -- zlib.compressobj(level, DEFLATED, wbits, 8, 0), each
piece fed in 32,768-byte compress() calls as the reference's stream layer feeds deflate
(streams.ts:7,78-84), flush(Z_FULL_FLUSH) at each flush position, flush() at the end, a gzip
header's OS byte patched to 0xff (the engine writes OS_CODE 255, deflate.ts:799).  A
deflate-raw case also lists the offsets behind its markers, where a decoder can restart.

zlib 1.2.11 is the yardstick because the reference's stream layer never passes a flush mode
other than Z_NO_FLUSH and Z_FINISH; SURVEY F5 found zlib 1.2.11 byte-identical to the
reference for levels 1-9 in all three formats, and deflate.ts:942-955 reads line for line as
zlib's deflate().  Other zlib versions differ in deflate_fast / deflate_slow details, so this
script refuses to run on them.  Every output is inflated back and compared with its input, and
must stay within zs_deflate_bound_flush.

    python tests/golden/gen_deflate_flush.py            # rewrite the file
    python tests/golden/gen_deflate_flush.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import flushcases as cases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    out = {}
    for c in cases.all_cases():
        name, data, level, fmt, pos = c
        assert name not in out, name
        y = cases.yardstick(c)
        assert zlib.decompress(y, cases.WBITS[fmt]) == data, name
        assert len(y) <= cases.bound(len(data), fmt, len(pos)), name
        out[name] = cases.entry(c)
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
