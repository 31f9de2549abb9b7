"""Inputs and helpers of the multi-member gzip tests (test_members_host.py, test_gpu_inflate_members.py):
members made with Python's zlib and with hand-made headers, the yardstick that walks a file's members
with zlib.decompressobj(31) by the rule of include/zs_gpu.h, and the host stand-in tools/members_host,
which runs the scan's candidate rule, the sizing lanes and the plan on the CPU."""
import os
import struct
import subprocess
import zlib

import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tools", "members_host")
FINAL, ERROR, PASSED = 2, 3, 4
# the BGZF end-of-file marker (SAM/BAM specification, section 4.1.2): an empty member with a BC subfield
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
assert len(BGZF_EOF) == 28
CAPACITY = (-5, 0, "output capacity exceeded")  # ZS_BUF_ERROR, ZS_PHASE_NONE, the message


def text(n, seed=7):
    return corpus.text(corpus.stream_seed(seed), n)


def cap4(n):
    return (n + 3) & ~3


def member(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def raw(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def trailer(data):
    return struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def hand_member(data, extra=None, name=None, comment=None, fhcrc=False, level=6):
    """a member whose header is built by hand: FEXTRA (`extra`: the field's bytes), FNAME, FCOMMENT, FHCRC"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    hdr = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\xff"
    if extra is not None:
        hdr += struct.pack("<H", len(extra)) + extra
    if name is not None:
        hdr += name + b"\x00"
    if comment is not None:
        hdr += comment + b"\x00"
    if fhcrc:
        hdr += struct.pack("<H", zlib.crc32(hdr) & 0xffff)
    return hdr + raw(data, level) + trailer(data)


def bc_extra(bsize=0):
    """the BGZF subfield: SI1 'B', SI2 'C', SLEN 2, BSIZE"""
    return b"BC" + struct.pack("<HH", 2, bsize)


def is_start(s, p):
    """the four-byte test of a member's start (include/zs_gpu.h)"""
    return p + 4 <= len(s) and s[p:p + 3] == b"\x1f\x8b\x08" and (s[p + 3] & 0xe0) == 0


def candidates(s):
    """the scan's rule, from the bytes: every q >= 1 that passes the four-byte test"""
    return [q for q in range(1, len(s)) if is_start(s, q)]


def walk(s):
    """The yardstick: a decompressobj(31) per member, restarted on unused_data while that begins with a
    member's start.  Returns (index [(in_pos, out_pos)] of every member met, the output of the complete
    members, where the stream ended -- consumed -- or the failing member's start, whether all decoded)."""
    pos, out, idx = 0, b"", []
    while True:
        idx.append((pos, len(out)))
        d = zlib.decompressobj(31)
        try:
            o = d.decompress(s[pos:])
        except zlib.error:
            return idx, out, pos, False
        if not d.eof:
            return idx, out, pos, False
        out += o
        pos = len(s) - len(d.unused_data)
        if not is_start(s, pos):
            return idx, out, pos, True


def good(s):
    """the fields of a stream whose members all decode: (status, phase, msg, bytes, consumed, check)"""
    idx, out, pos, ok = walk(s)
    assert ok
    return (1, 0, "", out, pos, zlib.crc32(out))


def stored_gz_case(inner=12, seed=0):
    """One level-0 member whose stored data is `inner` tiny complete .gz files (each a false candidate that sizes as a
    member), followed by one ordinary member: (the stream, the source, the second member's start)"""
    files = b"".join(member(text(5 + k, seed + k)) for k in range(inner))
    first = member(files, 0)
    tail = text(300, seed + 99)
    return first + member(tail), files + tail, len(first)


def bgzf(data, block=65280, level=6):
    return b"".join(hand_member(data[a:a + block], extra=bc_extra(), level=level) for a in range(0, len(data), block)) + BGZF_EOF


def build(name="members_host"):
    subprocess.check_call(["make", "-s", "-C", HOST, name])
    return os.path.join(HOST, name)


def _blob(streams, caps):
    return struct.pack("<I", len(streams)) + b"".join(struct.pack("<II", len(s), c) + s for s, c in zip(streams, caps))


def run(exe, streams, sync_pass=8, caps=None):
    """[(candidates, records, tail rounds, in_place, members)]: records [(how, end, len, reach)] of offset
    0's lane and of every candidate's, as the bounded lanes left them; members [(in_pos, in_len, out_pos,
    cap)] as zs_plan_members lays them out after the tail rounds"""
    caps = caps or [0xffffffff] * len(streams)
    r = subprocess.run([exe, str(sync_pass), "0"], input=_blob(streams, caps), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for _ in streams:
        C, = struct.unpack_from("<I", o, at)
        at += 4
        cand = list(struct.unpack_from("<%dI" % C, o, at))
        at += 4 * C
        recs = [struct.unpack_from("<4I", o, at + 16 * k) for k in range(C + 1)]
        at += 16 * (C + 1)
        rounds, in_place, P = struct.unpack_from("<3I", o, at)
        at += 12
        mem = [struct.unpack_from("<4I", o, at + 16 * k) for k in range(P)]
        at += 16 * P
        res.append((cand, recs, rounds, in_place, mem))
    assert at == len(o)
    return res


def run_every_offset(exe, streams):
    """[records]: a lane from every byte offset of every stream, bounded by the stream's end"""
    r = subprocess.run([exe, "8", "1"], input=_blob(streams, [0] * len(streams)), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for s in streams:
        res.append([struct.unpack_from("<4I", o, at + 16 * k) for k in range(len(s))])
        at += 16 * len(s)
    assert at == len(o)
    return res
