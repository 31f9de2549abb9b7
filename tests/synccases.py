"""Inputs and helpers of the restart-point search's tests (test_sync_host.py, test_gpu_inflate_sync.py):
streams made with Python's zlib, whose own bytes give every expectation, and the host stand-in
tools/sync_host, which runs the scan's candidate rule, the count-only decode and the plan on the CPU."""
import os
import struct
import subprocess
import zlib

import corpus
from restartcases import WBITS, flushed, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tools", "sync_host")
M = b"\x00\x00\xff\xff"
LANDED, FINAL, ERROR, PASSED = 1, 2, 3, 4


def build(name="sync_host"):
    subprocess.check_call(["make", "-s", "-C", HOST, name])
    return os.path.join(HOST, name)


def _blob(streams):
    return struct.pack("<I", len(streams)) + b"".join(struct.pack("<I", len(s)) + s for s in streams)


def run(exe, streams, fmt, sync_pass=8):
    """[(first, candidates, records, points)]: records [(how, end, len, reach)] of the first point's lane
    and of every candidate's; points [(in_pos, out_pos)] as zs_plan_sync emits them, the first included"""
    r = subprocess.run([exe, str(WBITS[fmt]), str(sync_pass), "0"], input=_blob(streams), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for _ in streams:
        first, C = struct.unpack_from("<2I", o, at)
        at += 8
        cand = list(struct.unpack_from("<%dI" % C, o, at))
        at += 4 * C
        recs = [struct.unpack_from("<4I", o, at + 16 * k) for k in range(C + 1)]
        at += 16 * (C + 1)
        P, = struct.unpack_from("<I", o, at)
        at += 4
        pts = [struct.unpack_from("<2I", o, at + 8 * k) for k in range(P)]
        at += 8 * P
        res.append((first, cand, recs, pts))
    assert at == len(o)
    return res


def run_every_offset(exe, streams, fmt):
    """[(first, records)]: a lane from every byte offset of every stream, bounded by the stream's end"""
    r = subprocess.run([exe, str(WBITS[fmt]), "8", "1"], input=_blob(streams), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for s in streams:
        first, = struct.unpack_from("<I", o, at)
        at += 4
        res.append((first, [struct.unpack_from("<4I", o, at + 16 * k) for k in range(len(s))]))
        at += 16 * len(s)
    assert at == len(o)
    return res


def candidates(stream, first):
    """the scan's rule, from the bytes: every q with stream[q-4:q] == M, first + 4 <= q <= len"""
    out, at = [], stream.find(M, first)
    while at >= 0:
        out.append(at + 4)
        at = stream.find(M, at + 1)
    return out


def mixed(data, flushes, fmt="deflate-raw", level=6):
    """`data` compressed with a flush of the given kind at each (position, kind) of `flushes`: the stream
    and [(in_pos, out_pos, kind)]"""
    co = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    out, idx, at = b"", [], 0
    for p, kind in flushes:
        out += co.compress(data[at:p]) + co.flush(kind)
        idx.append((len(out), p, kind))
        at = p
    out += co.compress(data[at:]) + co.flush()
    return out, idx


def full_points(idx):
    return [(a, b) for a, b, kind in idx if kind == zlib.Z_FULL_FLUSH]


def repeated_text(n):
    """text whose later parts copy from its earlier ones: a sync flush inside it leaves a window that is used"""
    base = text(700, 9)
    return (base * (n // len(base) + 1))[:n]


def gzip_with_fields(raw, data, extra, name):
    """a gzip member with an FEXTRA and an FNAME field around the raw deflate stream `raw` of `data` (a
    name ends at its first zero byte, so only the extra field can hold the marker's bytes)"""
    hdr = b"\x1f\x8b\x08\x0c\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(extra)) + extra + name + b"\x00"
    return hdr + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff), len(hdr)


def pass_case(K):
    """level 0: a piece whose data holds K + 2 copies of the marker between two true flushes"""
    d = text(50, 1) + M * (K + 2) + b"xyz" + text(50, 2)
    s, idx = flushed(d, [50, 50 + 4 * (K + 2) + 3], "deflate-raw", 0)
    return d, s, idx


FALSE_SOURCES = (
    # (source, flush position, level, raw candidates, the index of the true one)
    (b"abc" + M + b"defg" + M * 3 + text(200), 50, 0, 5, 4),
    (corpus.rand(11, 500) + M + corpus.rand(12, 500), 300, 6, 2, 0),
)


def passed_sync_case():
    """A raw stream put together from three pieces: text closed by a Z_SYNC_FLUSH; one stored block whose data
    holds 12 copies of the marker; text compressed against the bytes before it, so its copies reach back across
    both.  The lane that starts behind the sync flush is stopped by its bound (sync_pass 8) inside the stored
    block with a reach of 0: only the rest of the tail shows that the window behind that point is in use."""
    head = repeated_text(1400)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    a = co.compress(head) + co.flush(zlib.Z_SYNC_FLUSH)
    junk = b"".join(corpus.rand(k, 9) + M for k in range(12))
    b = b"\x00" + struct.pack("<HH", len(junk), len(junk) ^ 0xffff) + junk
    rest = repeated_text(1500)
    cz = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=head + junk)
    c = cz.compress(rest) + cz.flush()
    data, stream = head + junk + rest, a + b + c
    assert zlib.decompress(stream, -15) == data
    return data, stream, len(a)
