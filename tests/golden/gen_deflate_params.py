#!/usr/bin/env python3
"""Writes tests/golden/deflate_params.json: (length, sha256[:16]) of what C zlib 1.2.11
produces for every case of tests/paramcases.py -- zlib.compressobj(level, DEFLATED, wbits,
mem_level, 0) fed in 32,768-byte compress() calls and then flush(), as the reference's
stream layer feeds deflate (streams.ts:7,78-84), a gzip header's OS byte patched to 0xff
(the engine writes OS_CODE 255, deflate.ts:799).

zlib 1.2.11 is the yardstick because the CPU oracle is fixed at memLevel 8 / windowBits 15
and the reference's distributed bundle exports only the two stream classes, which never
pass other values; SURVEY F5 found zlib 1.2.11 byte-identical to the reference for levels
1-9 in all three formats.  Other zlib versions differ in deflate_fast / deflate_slow
details, so this script refuses to run on them.

zlib 1.2.11 predates the pending-buffer fix of 1.2.12: with a small memLevel it can
overwrite symbols it has not yet coded and emit a corrupt stream.  A case it corrupts is no
yardstick, so every output is inflated back and compared with its input here; pick other
cases rather than dropping the assert.

    python tests/golden/gen_deflate_params.py            # rewrite the file
    python tests/golden/gen_deflate_params.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import paramcases as cases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    out = {}
    for c in cases.all_cases():
        name, data, level, fmt, window_bits, mem_level = c
        assert name not in out, name
        y = cases.yardstick(c)
        # (window_bits 8 runs as 9 and says so in its header: a 256-byte inflate window refuses it)
        assert zlib.decompress(y, cases.wbits_code(fmt, max(window_bits, 9))) == data, "zlib corrupts %s: no yardstick" % name
        assert len(y) <= cases.bound(len(data), fmt, window_bits, mem_level, level), name
        out[name] = cases.digest(y)
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
