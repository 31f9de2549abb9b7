#!/usr/bin/env python3
"""Writes tests/golden/deflate_strategy.json: (length, sha256[:16]) of what C zlib
1.2.11 produces for every case of tests/strategycases.py --
zlib.compressobj(level, DEFLATED, wbits, 8, strategy), one compress() + flush(), a
gzip header's OS byte patched to 0xff (the engine writes OS_CODE 255, deflate.ts:799).

zlib 1.2.11 is the yardstick because the reference's distributed bundle exports
only the two stream classes, which always run strategy 0, and SURVEY F5 found zlib
1.2.11 byte-identical to the reference for levels 1-9 in all three formats; other
zlib versions differ in deflate_fast / deflate_slow details and in _tr_flush_block's
Z_FIXED test, so this script refuses to run on them.

Z_RLE has two sets.  The cases named .../ref0 are zlib's Z_RLE (option rle_ref = 0).
The cases named .../ref1 (the default: the reference) hold zlib's Z_HUFFMAN_ONLY
bytes: that equality is not measured on the reference but rests on reading
deflate.ts:1469-1481, where deflate_rle compares the previous byte's VALUE with the
scan INDEX three times in a row (prev == ++scan), which cannot hold, so no run is
ever found and the tally is deflate_huff's; the wrapper bits test strategy >= 2 for
both (deflate.ts:757,798).

Z_FIXED: the reference takes the static length whatever the dynamic one before the
stored test (trees.ts:567, zlib >= 1.2.12), zlib 1.2.11 only behind it; the two
differ where a block's stored length lies between them, which no case here does
(text and zeros: static far below stored; random bytes: both above stored).

    python tests/golden/gen_deflate_strategy.py            # rewrite the file
    python tests/golden/gen_deflate_strategy.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import strategycases as cases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    out = {}
    for c in cases.all_cases():
        assert c[0] not in out, c[0]
        out[c[0]] = cases.digest(cases.yardstick(c))
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
