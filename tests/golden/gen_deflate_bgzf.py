#!/usr/bin/env python3
"""Writes tests/golden/deflate_bgzf.json: (length, sha256[:16]) of every case of tests/bgzfwritecases.py -- the
BGZF framing of include/zs_gpu.h round each piece's zlib.compressobj(level, DEFLATED, -15, 8, 0) output from C
zlib 1.2.11, one compress() of the whole piece and flush() (what htslib's bgzf_compress does); level 0 by hand.

zlib 1.2.11 is the yardstick because it is byte-identical to the reference for levels 1-9; for a
piece of at most 65,280 bytes one-shot Z_FINISH and the stream layer's 32 KiB feeding give the same bytes.
Other zlib versions differ in deflate_fast / deflate_slow details, so this script refuses to run on them.
Every output is inflated back and compared with its input, and must stay within zs_deflate_bound_bgzf.

    python tests/golden/gen_deflate_bgzf.py            # rewrite the file
    python tests/golden/gen_deflate_bgzf.py --check    # compare, exit 1 on a difference
"""
import gzip
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bgzfwritecases as cases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    out = {}
    for c in cases.all_cases():
        name, data, level, block_bytes = c
        assert name not in out, name
        y = cases.yardstick(c)
        assert gzip.decompress(y) == data, name
        assert len(y) <= cases.bound(len(data), block_bytes), name
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
