"""Inputs and helpers of the BGZF fast path's tests (test_bgzf_host.py, test_capi_bgzf.py, test_gpu_inflate_bgzf.py):
BGZF blocks whose BSIZE is filled in (memberscases.bgzf() leaves BSIZE 0, which no reader can follow: those blocks
are members like any other and are covered as such), blocks whose headers lie, the rule of a TRUSTED header written
out in Python from include/zs_gpu.h, and the host stand-in tools/bgzf_host, which runs the scan's rule, zs_bgzf.h's
lane, the plan and the trusted flags on the CPU."""
import os
import struct
import subprocess
import zlib

import memberscases as mc
from memberscases import BGZF_EOF, bc_extra, hand_member, text  # noqa: F401

HOST = os.path.join(mc.ROOT, "tools", "bgzf_host")
ISIZE_MAX = 65536


def block(data, front=b"", back=b"", level=6, bsize_delta=0, isize=None):
    """one BGZF block: FLG 4, the extra field `front` + BC + `back`, BSIZE = the block's size - 1 (+ bsize_delta: a
    lie), the trailer's ISIZE (isize: a lie)"""
    at = 12 + len(front) + 4
    b = bytearray(hand_member(data, extra=front + bc_extra(0) + back, level=level))
    struct.pack_into("<H", b, at, len(b) - 1 + bsize_delta)
    if isize is not None:
        struct.pack_into("<I", b, len(b) - 4, isize)
    return bytes(b)


def bgzf(data, block_bytes=65280, level=6, eof=True):
    """a BGZF file as bgzip writes it: blocks of block_bytes, then the end-of-file block"""
    return b"".join(block(data[a:a + block_bytes], level=level) for a in range(0, len(data), block_bytes)) + (BGZF_EOF if eof else b"")


def trusted(s, p):
    """the rule of include/zs_gpu.h: (end, ISIZE) when the header at p can be trusted, else None"""
    n = len(s)
    if p + 18 > n or s[p:p + 4] != b"\x1f\x8b\x08\x04":
        return None
    xlen, = struct.unpack_from("<H", s, p + 10)
    x1 = p + 12 + xlen
    if x1 > n:
        return None
    at, bsize = p + 12, None
    while at + 4 <= x1:
        slen, = struct.unpack_from("<H", s, at + 2)
        if at + 4 + slen > x1:
            return None
        if bsize is None and s[at:at + 2] == b"BC" and slen == 2:
            bsize, = struct.unpack_from("<H", s, at + 4)
        at += 4 + slen
    if at != x1 or bsize is None:
        return None
    total = bsize + 1
    if total <= 12 + xlen + 8 or p + total > n:
        return None
    isize, = struct.unpack_from("<I", s, p + total - 4)
    return (p + total, isize) if isize <= ISIZE_MAX else None


def chain(s):
    """zs_bgzf_out_len's answer from the headers: (1, the sum of ISIZE) or (0, 0); and the index read from them"""
    p, total, idx = 0, 0, []
    while True:
        t = trusted(s, p)
        if t is None:
            return 0, 0, idx
        idx.append((p, total))
        p, total = t[0], total + t[1]
        if not mc.is_start(s, p):
            return 1, total, idx


def build(name="bgzf_host"):
    subprocess.check_call(["make", "-s", "-C", HOST, name])
    return os.path.join(HOST, name)


def run(exe, streams, sync_pass=8, caps=None):
    """[(candidates, records, tail rounds, in_place, members, (ok, total))]: records [(how, end, len, reach, trusted)]
    of offset 0's lane and of every candidate's; members [(in_pos, in_len, out_pos, cap, trusted)] as
    zs_plan_members lays them out after the tail rounds, with zs_plan_bgzf_trusted's flags; zs_bgzf_chain's answer"""
    caps = caps or [0xffffffff] * len(streams)
    r = subprocess.run([exe, str(sync_pass), "0"], input=mc._blob(streams, caps), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for _ in streams:
        C, = struct.unpack_from("<I", o, at)
        at += 4
        cand = list(struct.unpack_from("<%dI" % C, o, at))
        at += 4 * C
        recs = [struct.unpack_from("<5I", o, at + 20 * k) for k in range(C + 1)]
        at += 20 * (C + 1)
        rounds, in_place, P = struct.unpack_from("<3I", o, at)
        at += 12
        mem = [struct.unpack_from("<5I", o, at + 20 * k) for k in range(P)]
        at += 20 * P
        ok, total = struct.unpack_from("<IQ", o, at)
        at += 12
        res.append((cand, recs, rounds, in_place, mem, (ok, total)))
    assert at == len(o)
    return res


def run_every_offset(exe, streams):
    """[records]: a lane from every byte offset of every stream, bounded by the stream's end"""
    r = subprocess.run([exe, "8", "1"], input=mc._blob(streams, [0] * len(streams)), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    o, at, res = r.stdout, 0, []
    for s in streams:
        res.append([struct.unpack_from("<5I", o, at + 20 * k) for k in range(len(s))])
        at += 20 * len(s)
    assert at == len(o)
    return res


def xy_block(data):
    """a block whose extra field holds an XY subfield in front of BC (and one behind it)"""
    return block(data, front=b"XY\x03\x00abc", back=b"ZZ\x00\x00")


def crc_low_block():
    """A block whose data is 256 bytes (a multiple of 256) with a crc32 below 2^24: with BSIZE shortened by 3 the four
    bytes read as ISIZE are crc32 >> 8 and the length's low byte, at most 65,535 -- the shortened header is still
    TRUSTED.  (data, the block, the ISIZE the shortened header shows)"""
    for k in range(1 << 20):
        d = text(252, 9) + struct.pack("<I", k)
        c = zlib.crc32(d)
        if c < (1 << 24):
            return d, block(d), c >> 8
    raise AssertionError("no such data")
