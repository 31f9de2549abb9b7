"""GPU check of the inflate entries' refusals: the rows of tests/inflatefaultcases.py that have a context,
through the real entries (zs_inflate_batch_device, _dict_device, zs_inflate_batch_ex, _dict), two tiny
members each.  A refusal gives the table's code and message and leaves the result arrays and the output
bytes alone; a good call on the same engine straight afterwards decodes, and its counters are its own."""
import ctypes
import zlib

import pytest

import hostchunkcases as hc
import inflatefaultcases as fc
from test_plan_inflate_faults import real_call

pytestmark = pytest.mark.gpu

DATA = [b"", b"abc"]
DICT = b"hello"  # (shares no three bytes with b"abc": the member decodes without it too)
FILL = 0x5A


def members(wbits):
    def one(d):
        co = zlib.compressobj(6, zlib.DEFLATED, 31 if wbits == 31 else -15, **({} if wbits == 31 or not d else {"zdict": DICT}))
        return co.compress(d) + co.flush()

    return [b"\x03\x00" if wbits != 31 else one(b""), one(b"abc")]


def layout(items):
    offs, at = [], 0
    for b in items:
        offs.append(at)
        at += len(b)
    return b"".join(items) + bytes(8), offs


def test_refusals_and_the_call_after_them(engine):
    import torch

    L = engine._L
    total = 32
    canary = hc.canary(total)
    other = []
    for k in (1, 2000, 3):
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        other.append(co.compress(b"x" * k) + co.flush())

    def good(baseline=None):
        """the plain host call of the two members; its counters"""
        res = hc.inflate(engine, members(-15), "deflate-raw", [1, 3])
        assert (res["status"], res["data"]) == ([1, 1], DATA)
        got = (engine.last_host_chunks(), engine.last_checksum_parts(), engine.last_lane_count(), engine.last_seg_count())
        assert baseline is None or got == baseline
        return got

    with hc.options(engine, checksum_split=1, checksum_part=1024):
        baseline = good()
        assert baseline[:2] == (1, 0) and baseline[3] == 0
        refused = 0
        for row in fc.rows():
            a = fc.arguments(row)
            if not a["ctx"]:
                continue
            blob, ioffs = layout(members(a["wbits"]))
            for kind in fc.KINDS:
                want = fc.expected(kind, row)
                n = a["n"]
                mem = {"in_off": ioffs[:n], "in_len": [len(m) for m in members(a["wbits"])][:n], "dict_off": [0] * n}
                if kind.endswith("device"):
                    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
                    d_out = torch.frombuffer(bytearray(canary), dtype=torch.uint8).cuda()
                    d_res = torch.full((6, 2), FILL * 0x01010101, dtype=torch.int32, device="cuda")
                    d_dict = torch.frombuffer(bytearray(DICT + bytes(3)), dtype=torch.uint8).cuda()
                    mem.update({"in": d_in.data_ptr(), "out": d_out.data_ptr(), "dict": d_dict.data_ptr(),
                                "res": [ctypes.c_void_p(d_res[r].data_ptr()) for r in range(6)]})
                else:
                    out = ctypes.create_string_buffer(canary, total)
                    res = [(ctypes.c_int32 * 2)() for _ in range(3)] + [(ctypes.c_uint32 * 2)() for _ in range(3)]
                    for r in res:
                        ctypes.memset(r, FILL, 8)
                    mem.update({"in": blob, "out": out, "dict": DICT, "res": res})
                if want != "ok":
                    # a call with other counters first: three gzip members, four checksum parts
                    hc.inflate(engine, other, "gzip", [1, 2000, 3])
                    assert engine.last_checksum_parts() == 4
                rc = real_call(L, kind, a, engine.handle, mem)
                if kind.endswith("device"):
                    torch.cuda.synchronize()
                    got_out = bytes(d_out.cpu().numpy().tobytes())
                    got_res = [[int(x) for x in d_res[r].cpu().tolist()] for r in range(6)]
                else:
                    got_out, got_res = out.raw, [list(r) for r in res]
                if want == "ok":
                    assert rc == 0, (row, kind, L.zs_last_error())
                    if n:
                        checked = 6 if kind != "device" else 5  # (zs_inflate_batch_device takes no check array)
                        assert got_res[0] == [1, 1] and got_res[3] == [0, 3], (row, kind, got_res)
                        assert got_out[a["offs"][1]:a["offs"][1] + 3] == b"abc", (row, kind)
                        assert all(FILL * 0x01010101 not in r for r in got_res[:checked])
                    continue
                refused += 1
                assert (rc, L.zs_last_error().decode()) == (fc.ZS_STREAM_ERROR, fc.MESSAGES[want]), (row, kind)
                assert got_out == canary, (row, kind)
                assert all(x == FILL * 0x01010101 for r in got_res for x in r), (row, kind)
                good(baseline)
        assert refused > 100
