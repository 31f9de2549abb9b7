"""GPU tests of what the entries that find a stream's pieces share on a context (capi.cpp: cand_search's
buffers and candidate list, the pieces' buffers): calls of every kind, one after the other on ONE context,
give what each gives alone on a fresh context, and the candidate list grows through either kind.  The
streams come from the helpers of each entry's own tests (restartcases, synccases, memberscases, bgzfcases)."""
import contextlib
import zlib

import pytest

import bgzfcases
import memberscases as mc
import synccases
from memberscases import member
from restartcases import cap4, flushed, text

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def fresh_engine():
    import torch

    if torch.cuda.is_available():  # (torch's HIP runtime first, as conftest's engine: later tests hand it device buffers)
        torch.cuda.init()
    import zsamd

    eng = zsamd.Engine()
    try:
        yield eng
    finally:
        eng.close()


def record(eng, **call):
    """a call's six fields per stream, and the three records the context keeps of its last call"""
    got = eng.decompress_batch_detailed(**call)
    return got, eng.last_restart_points(), eng.last_members(), eng.last_bgzf_trusted()


def test_calls_of_every_kind_on_one_context_give_what_each_gives_alone():
    # three zlib streams of about 4 KiB with a full-flush point every 1 KiB
    datas = [text(4096 + 40 * k, 11 + k) for k in range(3)]
    made = [flushed(d, [1024, 2048, 3072], "deflate") for d in datas]
    zstreams, zpoints = [s for s, _ in made], [p for _, p in made]
    zcaps = [cap4(len(d)) + 8 for d in datas]
    # three gzip streams of 2, 1 and 5 members
    parts = [[text(700 + 13 * j, 20 + 8 * k + j) for j in range(m)] for k, m in enumerate((2, 1, 5))]
    gstreams = [b"".join(member(p) for p in ps) for ps in parts]
    gcaps = [sum(len(p) for p in ps) + 8 for ps in parts]
    # a BGZF file of six 1 KiB blocks; three ranges over it, the first one ending inside a block
    bdata = text(6144, 31)
    bfile = bgzfcases.bgzf(bdata, 1024)
    starts = [a for a, _ in mc.walk(bfile)[0]]
    assert len(starts) == 7  # (the end-of-file block last)
    ranges = [(starts[1] << 16 | 10, starts[3] << 16 | 500), (0, starts[2] << 16), (starts[4] << 16, starts[6] << 16)]
    wanted = [bdata[1024 + 10:3072 + 500], bdata[:2048], bdata[4096:]]
    sync = dict(inputs=zstreams, fmt="deflate", out_caps=zcaps, restart="scan")
    calls = [
        ("sync", sync, datas),
        ("members", dict(inputs=gstreams, fmt="gzip", out_caps=gcaps, members=True), [b"".join(ps) for ps in parts]),
        ("bgzf", dict(inputs=[bfile], fmt="gzip", out_caps=[cap4(len(bdata))], members="bgzf"), [bdata]),
        ("bgzf_range", dict(inputs=[bfile] * 3, fmt="gzip", members="bgzf", ranges=ranges), wanted),
        ("restart", dict(inputs=zstreams, fmt="deflate", out_caps=zcaps, restart=zpoints), datas),
        ("sync again", sync, datas),
    ]
    with fresh_engine() as eng:
        mixed = [record(eng, **call) for _, call, _ in calls]
    for (name, call, want), got in zip(calls, mixed):
        with fresh_engine() as eng:
            alone = record(eng, **call)
        assert got == alone, name
        assert [g[0] for g in got[0]] == [1] * len(want) and [g[3] for g in got[0]] == want, name
    assert mixed[0][1] == zpoints and mixed[5][1] == zpoints
    assert mixed[1][2] == [mc.walk(s)[0] for s in gstreams]
    assert mixed[2][3] > 0 and mixed[3][3] > 0


def test_the_candidate_list_grows_through_either_kind():
    """1,200 empty stored blocks are 1,200 restart candidates in 6 KiB, more than the list a context starts with
    (1,024 and one per 2 KiB of input, and an eighth on top: the buffers' growth step), so the emit pass and
    the sizing run once more over the grown list; the members' growth stream on the same context then outgrows
    that list again"""
    s = b"\x00\x00\x00\xff\xff" * 1200 + b"\x01\x04\x00\xfb\xfftail"
    room = 4 * (len(s) // 2048 + 1024)
    assert len(synccases.candidates(s, 0)) == 1200 > (room + room // 8) // 4
    g = member(b"\x1f\x8b\x08\x00" * 5000, 0) + member(b"tail")
    assert len(mc.candidates(g)) == 5001
    mcall = dict(inputs=[g], fmt="gzip", out_caps=[20008], members=True)
    with fresh_engine() as eng:
        (got,) = eng.decompress_batch_detailed([s], "deflate-raw", out_caps=[8], restart="scan")
        assert got[:5] == (1, 0, "", b"tail", len(s))
        grown = record(eng, **mcall)
    with fresh_engine() as eng:
        assert grown == record(eng, **mcall)
    assert grown[0] == [(1, 0, "", b"\x1f\x8b\x08\x00" * 5000 + b"tail", len(g), zlib.crc32(b"\x1f\x8b\x08\x00" * 5000 + b"tail"))]
