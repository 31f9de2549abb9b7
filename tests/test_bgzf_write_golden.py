"""CPU: the BGZF writer's yardstick (tests/bgzfwritecases.py) against the committed goldens
(tests/golden/deflate_bgzf.json) and against everything else that reads a BGZF file here: gzip.decompress, the
trusted-header rule and the chain of the BGZF reader's tests (bgzfcases), the reference's restatement of deflate
(oracle.compress) for the pieces' bytes, zs_deflate_bound_bgzf, and the 16-bit BSIZE."""
import gzip
import struct
import zlib

import pytest

import bgzfcases
import bgzfwritecases as w
import oracle


@pytest.fixture(scope="module")
def outputs():
    return {c[0]: w.yardstick(c) for c in w.all_cases()}


def test_the_goldens_cover_the_cases():
    assert sorted(w.golden()) == sorted(c[0] for c in w.all_cases())
    assert len(w.all_cases()) == len(set(c[0] for c in w.all_cases())) >= 30


def test_the_yardstick_is_the_committed_golden_where_zlib_1_2_11_runs(outputs):
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        pytest.skip("the goldens are zlib 1.2.11's; zlib %s is running" % zlib.ZLIB_RUNTIME_VERSION)
    g = w.golden()
    assert {k: w.digest(v) for k, v in outputs.items()} == g


def test_every_output_gunzips_back_to_its_input(outputs):
    for c in w.all_cases():
        assert gzip.decompress(outputs[c[0]]) == c[1], c[0]


def test_every_block_header_is_trusted_and_the_chain_reaches_the_end(outputs):
    for c in w.all_cases():
        name, data, level, bb = c
        y = outputs[name]
        ok, total, idx = bgzfcases.chain(y)
        assert (ok, total) == (1, len(data)), name
        assert [(o, i) for i, o in w.index(data, level, bb)] == idx, name  # chain's (offset in the file, bytes before)
        assert idx[-1][0] == len(y) - 28 and y[-28:] == w.EOF, name
        for p, _ in idx:
            end, isize = bgzfcases.trusted(y, p)
            assert end - p <= 65536, name
            assert y[p:p + 16] == w.HEADER and struct.unpack_from("<H", y, p + 16)[0] == end - p - 1, name
            assert y[p + 8] == 0, name  # XFL 0 at every level


def test_every_output_is_within_the_bound(outputs):
    room = [w.bound(len(c[1]), c[3]) - len(outputs[c[0]]) for c in w.all_cases()]
    assert min(room) >= 0
    assert w.bound(0) == 28 and w.bound(1) == 8 + 26 + 28 and w.bound(w.B) == 65305 + 26 + 28 <= 65536 + 28


def subset():
    """one case per group and level: short ones whole, of the long ones the first and the last piece"""
    seen, out = set(), []
    for c in w.all_cases():
        key = (c[0].split("/")[0], c[2])
        if key not in seen and c[2] != 0 and c[1]:
            seen.add(key)
            out.append(c)
    return out


def test_the_pieces_are_the_reference_restatements_raw_streams(outputs):
    """ties the goldens to the reference's restatement of deflate, not only to zlib"""
    cases = subset()
    assert len(cases) >= 12
    for name, data, level, bb in cases:
        ps = w.pieces(data, bb)
        for p in (ps[0], ps[-1]):
            st, raw = oracle.compress(p, level, "deflate-raw")[:2]
            assert raw == w.piece_raw(p, level), (name, len(p))
            assert w.member(p, level)[18:-8] == raw


def test_level_0_is_one_final_stored_block_per_piece(outputs):
    for name, data, level, bb in w.group("level0"):
        y, at = outputs[name], 0
        for p in w.pieces(data, bb):
            assert y[at + 18:at + 23] == b"\x01" + struct.pack("<HH", len(p), 0xffff - len(p)), name
            assert y[at + 23:at + 23 + len(p)] == p
            at += len(p) + 31
        assert y[at:] == w.EOF


def test_the_cut_piece_keeps_its_empty_static_block():
    import deflate_header

    x = w.filler(w.CUT)
    blocks = deflate_header.parse(w.piece_raw(x, 1))
    assert [b.type for b in blocks][-1] == 1 and len(blocks) == 2  # the full block, then the empty static one
