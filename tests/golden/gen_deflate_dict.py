#!/usr/bin/env python3
"""Writes tests/golden/deflate_dict.json: (length, sha256[:16]) of what C zlib
1.2.11 produces for every case of tests/deflatedictcases.py --
zlib.compressobj(level, DEFLATED, wbits, 8, 0, zdict), one compress() + flush().

zlib 1.2.11 is the yardstick because deflate.ts:367-424 follows its
deflateSetDictionary line for line and SURVEY F5 found it byte-identical to the
reference for levels 1-9 in all three formats; other zlib versions differ in
deflate_fast / deflate_slow details, so this script refuses to run on them.

    python tests/golden/gen_deflate_dict.py            # rewrite the file
    python tests/golden/gen_deflate_dict.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import deflatedictcases as cases  # noqa: E402
import dictcases  # noqa: E402

WANT_ZLIB = "1.2.11"


def generate():
    if zlib.ZLIB_RUNTIME_VERSION != WANT_ZLIB:
        raise SystemExit("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, WANT_ZLIB))
    out = {}
    for name, data, zdict, level, fmt in cases.all_cases():
        assert name not in out, name
        out[name] = cases.digest(dictcases.compress(data, level, fmt, zdict))
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
