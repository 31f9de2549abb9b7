"""The one table of what the inflate entries refuse and which fault wins (csrc/zs_plan.h:
zs_inflate_validate for a device batch, zs_inflate_validate_host for what a host entry decides
before it stages anything).  test_plan_inflate_faults.py runs it through tools/emu/emu_plan_inflate.cpp
and, its null-context rows, through the real entries; test_gpu_inflate_faults.py runs the others
through the real entries on the GPU.

A row is a good call of two tiny members with some of FAULTS put in, for each of the four KINDS of
entry.  `expected` states the order the entries report them in, as include/zs_gpu.h and the entries
have it:
  device (zs_inflate_batch_device[_ex], _dict_device, each chunk of a host call):
    null context; windowBits, even of an empty batch; with a dictionary argument and streams: null
    arrays, a length without a buffer, a length with gzip or deflate64; an empty batch is done;
    offsets (caller's regions: capacities too) that are no multiples of 4.
  host (zs_inflate_batch[_ex]): null context; an empty batch is done whatever windowBits is; the
    device order (the staging's regions are the entry's own: alignment is never the caller's fault).
  dict host (zs_inflate_batch_dict): null context; null arrays, even of an empty batch; an empty
    batch is done; the buffer; gzip or deflate64; then windowBits."""
import itertools

ZS_STREAM_ERROR = -2
# verdict -> zs_last_error(), in zs_inflate_err's order
MESSAGES = {
    "ok": "",
    "null_context": "null context",
    "wbits": "unsupported windowBits (use -15, 15, 31 or -16)",
    "dict_arrays": "null dictionary arrays",
    "dict_buffer": "null dictionary buffer",
    "dict_format": "dictionaries are for deflate-raw (-15) and zlib (15) only",
    "align": "output offsets/capacities must be multiples of 4",
}
VERDICTS = list(MESSAGES)
KINDS = ("device", "host", "dict_device", "dict_host")
# what a row can put into the good call; "gzip" and "d64" are faults only beside a dictionary's length
FAULTS = ("null_ctx", "wbits", "gzip", "d64", "dict_arrays", "dict_buffer", "align_off", "align_cap")
SETS_WBITS = {"wbits": 14, "gzip": 31, "d64": -16}
# ... and what changes which of them can show: no streams; every dictionary length 0
MODIFIERS = ("empty", "lens0")


def arguments(row):
    """the call of a row: ctx (a context is given), wbits, n, the dictionary arrays / buffer given and
    the lengths, the output offsets and capacities"""
    n = 0 if "empty" in row else 2
    wb = [v for k, v in SETS_WBITS.items() if k in row]
    offs, caps = [0, 6 if "align_off" in row else 8], [7 if "align_cap" in row else 4, 8]
    return {"ctx": "null_ctx" not in row, "wbits": wb[0] if wb else -15, "n": n, "arrays": "dict_arrays" not in row,
            "buf": "dict_buffer" not in row, "lens": ([0, 0] if "lens0" in row else [0, 5])[:n], "offs": offs[:n],
            "caps": caps[:n]}


def expected(kind, row):
    """the verdict of the entry kind for the row"""
    dic, host = kind.startswith("dict"), kind.endswith("host")
    streams = "empty" not in row
    # a dictionary's length counts once the arrays are there to read it from
    length = dic and streams and "lens0" not in row and "dict_arrays" not in row
    of_dict = [("dict_buffer", length and "dict_buffer" in row), ("dict_format", length and ("gzip" in row or "d64" in row))]
    device = ([("wbits", "wbits" in row), ("dict_arrays", dic and streams and "dict_arrays" in row)] + of_dict +
              [("ok", not streams), ("align", not host and ("align_off" in row or "align_cap" in row))])
    order = [("null_context", "null_ctx" in row)]
    if host and dic:
        order += [("dict_arrays", "dict_arrays" in row), ("ok", not streams)] + of_dict
    elif host:
        order += [("ok", not streams)]
    return next((v for v, hit in order + device if hit), "ok")


def rows():
    """no fault, every fault alone, every pair that can stand together; each of them with no streams too;
    the dictionary's faults with every length 0"""
    base = [()] + [(f,) for f in FAULTS] + [
        p for p in itertools.combinations(FAULTS, 2) if sum(f in SETS_WBITS for f in p) < 2]
    out = base + [r + ("empty",) for r in base]
    out += [r + ("lens0",) for r in base if r and set(r) <= {"gzip", "d64", "dict_buffer", "wbits", "align_cap"}]
    return out


def name(row):
    return "+".join(row) or "good"


def emu_lines():
    """the emulator's input: one line per row and per entry with / without a dictionary argument"""
    lines = []
    for row in rows():
        a = arguments(row)
        for dic in (0, 1):
            lists = [",".join(map(str, a[k])) or "-" for k in ("lens", "offs", "caps")]
            lines.append(" ".join([name(row) + ("/dict" if dic else "/plain"), str(int(a["ctx"])), str(a["wbits"]),
                                   str(a["n"]), str(dic), str(int(a["arrays"])), str(int(a["buf"]))] + lists))
    return lines


def emu_expected():
    """what the emulator prints for emu_lines(): name, then index and text of the device and the host verdict"""
    out = []
    for row in rows():
        for dic in (0, 1):
            v = [expected(("dict_" if dic else "") + where, row) for where in ("device", "host")]
            out.append("\t".join([name(row) + ("/dict" if dic else "/plain")] +
                                 [x for k in v for x in (str(VERDICTS.index(k)), MESSAGES[k])]))
    return out
