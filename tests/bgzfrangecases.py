"""Inputs and the model of the BGZF range tests (test_plan_bgzf_range.py, test_capi_bgzf_range.py,
test_gpu_inflate_bgzf_range.py, test_js_bgzf_range.py): virtual offsets (coffset << 16 | uoffset), the contract of
include/zs_gpu.h written out in Python over bgzfcases' rule of a trusted header, and the expected bytes from zlib
on the host -- the decompressed file sliced at the positions the virtual offsets name."""
import zlib

import bgzfcases as bc
import memberscases as mc
from memberscases import BGZF_EOF, CAPACITY, cap4, text  # noqa: F401

RANGE = (-3, 2, "virtual offsets do not follow a chain of BGZF blocks")  # ZS_DATA_ERROR, ZS_PHASE_PROCESS, the message
MEMBER_MAX = 65536


def voff(coffset, uoffset=0):
    return (coffset << 16) | uoffset


def blocks(s):
    """[(start, end, ISIZE)] of the trusted headers followed from 0 to where one is not trusted or the input ends"""
    p, out = 0, []
    while p < len(s):
        t = bc.trusted(s, p)
        if t is None:
            break
        out.append((p, t[0], t[1]))
        p = t[0]
    return out


def slice_of(s, vb, ve):
    """the bytes of the stream a range reads: (offset, length)"""
    cb, ce, ue = vb >> 16, ve >> 16, ve & 0xffff
    end = min(len(s), ce + MEMBER_MAX) if ue else ce
    return cb, end - cb


def plan(s, vb, ve):
    """The contract's chain, from the headers inside the slice: ("fail", the offending start), or ("ok", [(start,
    end, ISIZE, skip, take)] of the decoded members -- starts from the stream's beginning)."""
    assert vb <= ve and (ve >> 16) <= len(s)
    cb, ub, ce, ue = vb >> 16, vb & 0xffff, ve >> 16, ve & 0xffff
    off, n = slice_of(s, vb, ve)
    z = s[off:off + n]
    p, mem = cb, []
    while p < ce or (p == ce and ue):
        t = bc.trusted(z, p - cb)
        last = p == ce
        if t is None or (not last and cb + t[0] > ce):
            return "fail", p
        end, isize = cb + t[0], t[1]
        if (p == cb and ub > isize) or (last and ue > isize):
            return "fail", p
        skip = ub if p == cb else 0
        mem.append((p, end, isize, skip, (ue if last else isize) - skip))
        if last:
            break
        p = end
    return "ok", mem


def out_len(s, vb, ve):
    """zs_bgzf_range_out_len's answer: (1, the delivered length) or (0, 0)"""
    how, mem = plan(s, vb, ve)
    return (1, sum(m[4] for m in mem)) if how == "ok" else (0, 0)


def member_bytes(s, start, end):
    return zlib.decompressobj(31).decompress(s[start:end])


def expect(s, vb, ve, cap=None):
    """the fields (status, phase, msg, bytes, consumed, check) of a range over a stream whose blocks all decode and
    whose headers tell the truth; cap: the capacity (None: enough)"""
    how, mem = plan(s, vb, ve)
    if how == "fail":
        return RANGE + (b"", mem, 0)
    if not mem:
        return (1, 0, "", b"", vb >> 16, 0)
    out = b""
    for start, end, isize, skip, take in mem:
        if cap is not None and len(out) + take > cap:
            return CAPACITY + (out, start, 0)
        d = member_bytes(s, start, end)
        assert len(d) == isize
        out += d[skip:skip + take]
    return (1, 0, "", out, mem[-1][1], zlib.crc32(out))


def whole(s):
    """the uncompressed file and the index [(in_pos, out_pos)] of its blocks, the end entry included"""
    data, idx = b"", []
    for start, end, isize in blocks(s):
        idx.append((start, len(data)))
        data += member_bytes(s, start, end)
    return data, idx + [(blocks(s)[-1][1], len(data))]


def voffset(idx, upos):
    """zs_bgzf_voffset's answer over one stream's index: the last block with out_pos <= upos, or None"""
    if not idx or upos > idx[-1][1] or upos < idx[0][1]:
        return None
    k = max(i for i, (_, o) in enumerate(idx) if o <= upos)
    return voff(idx[k][0], upos - idx[k][1]) if upos - idx[k][1] <= 0xffff else None


def corners(s):
    """{name: (vb, ve)}: the range corners over a file of at least four data blocks and the end-of-file block"""
    b = blocks(s)
    assert len(b) >= 5 and b[-1][2] == 0 and b[-1][1] == len(s) and all(x[2] >= 1 for x in b[:-1])
    (s0, _, i0), (s1, _, i1), (s2, _, i2), (s3, _, _) = b[0], b[1], b[2], b[3]
    eof = b[-1][0]
    return {
        "one block, cb == ce": (voff(s1, 0), voff(s1, i1)),
        "inside one block": (voff(s1, min(1, i1)), voff(s1, i1 - (1 if i1 > 1 else 0))),
        "ub 0": (voff(s0, 0), voff(s2, 0)),
        "ub ISIZE": (voff(s0, i0), voff(s2, 0)),
        "ub ISIZE, cb == ce": (voff(s0, i0), voff(s0, i0)),
        "ue 0": (voff(s1, 0), voff(s2, 0)),
        "ue ISIZE": (voff(s1, 0), voff(s2, i2)),
        "ce at the end-of-file block": (voff(s1, 0), voff(eof, 0)),
        "ce == in_len": (voff(s1, 0), voff(len(s), 0)),
        "empty at a block": (voff(s2, 0), voff(s2, 0)),
        "empty at in_len": (voff(len(s), 0), voff(len(s), 0)),
        "2 blocks": (voff(s0, min(1, i0)), voff(s1, i1)),
        "3 blocks": (voff(s0, 0), voff(s2, max(i2 - 1, 1))),
        "the whole file": (0, voff(len(s), 0)),
    }


def header_failures(s):
    """{name: ((vb, ve), the offending start)} over the same kind of file"""
    b = blocks(s)
    (s0, _, i0), (s1, _, i1), (s2, _, i2) = b[0], b[1], b[2]
    return {
        "cb in the middle of a block": ((voff(s1 + 3, 0), voff(s2, 0)), s1 + 3),
        "ce in the middle of a block": ((voff(s0, 0), voff(s1 + 5, 0)), s1),
        "ce in the middle of a block, ue > 0": ((voff(s0, 0), voff(s1 + 5, 1)), s1),
        "ub above ISIZE": ((voff(s0, i0 + 1), voff(s2, 0)), s0),
        "ue above ISIZE": ((voff(s0, 0), voff(s2, i2 + 1)), s2),
        "ub above ISIZE, cb == ce": ((voff(s1, i1 + 1), voff(s1, i1 + 2)), s1),
        "ue > 0 at in_len": ((voff(s2, 0), voff(len(s), 1)), len(s)),
    }


def records(s, vb, ve, liar=True):
    """the slice's starts as the sizing launch leaves them: [(pos, how, end, len, trusted)], offset 0 first and then
    the scan's candidates; a start whose header is not trusted gets a record that claims a member all the same
    (liar), which the plan must not follow"""
    off, n = slice_of(s, vb, ve)
    z = s[off:off + n]
    out = []
    for p in [0] + mc.candidates(z):
        t = bc.trusted(z, p)
        if t is not None:
            out.append((p, mc.FINAL, t[0], t[1], 1))
        else:
            out.append((p, mc.FINAL, n, 5, 0) if liar else (p, mc.ERROR, p, 0, 0))
    return out
