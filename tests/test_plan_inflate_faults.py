"""CPU check of which fault of an inflate call wins (csrc/zs_plan.h: zs_inflate_validate,
zs_inflate_validate_host): tools/emu/emu_plan_inflate.cpp, plain g++, no ROCm headers, over the
table of tests/inflatefaultcases.py; once more as a stand-alone program under ASan + UBSan; and the
rows without a context through the real entries of libzsgpu.so, which need no GPU to refuse."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import inflatefaultcases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_inflate.cpp")
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Werror"]


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("emu")

    def make(name, extra=()):
        exe = str(d / name)
        r = subprocess.run(["g++", *FLAGS, *extra, "-o", exe, SRC], capture_output=True, text=True)
        return exe, r

    return make


def run(exe):
    r = subprocess.run([exe], input="\n".join(fc.emu_lines()) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_the_table_covers_what_it_is_meant_to():
    rows = fc.rows()
    assert len(rows) == len(set(rows))
    have = {frozenset(r) for r in rows}
    for f in fc.FAULTS:
        assert {f} in have and {f, "empty"} in have
    for a in fc.FAULTS:
        for b in fc.FAULTS:
            if a != b and not (a in fc.SETS_WBITS and b in fc.SETS_WBITS):
                assert {a, b} in have and {a, b, "empty"} in have
    # every verdict is reached, by every kind of entry that can give it
    for kind in fc.KINDS:
        seen = {fc.expected(kind, r) for r in rows}
        want = set(fc.VERDICTS)
        if kind.endswith("host"):
            want.discard("align")
        if not kind.startswith("dict"):
            want -= {"dict_arrays", "dict_buffer", "dict_format"}
        assert seen == want, kind


def test_the_fault_that_wins(build):
    exe, r = build("emu_plan_inflate")
    assert r.returncode == 0, r.stderr
    got, want = run(exe), fc.emu_expected()
    assert [g.split("\t")[0] for g in got] == [w.split("\t")[0] for w in want]
    for g, w in zip(got, want):
        assert g == w, w.split("\t")[0]
    verdict = {}
    for w in want:
        name, dev, _, host, _ = w.split("\t")
        verdict[name + "/device"], verdict[name + "/host"] = fc.VERDICTS[int(dev)], fc.VERDICTS[int(host)]
    # the distinctions between the entries, spelled out
    # ... an empty batch: the device entries still look at windowBits, the host entries do not
    assert verdict["wbits+empty/plain/device"] == "wbits" and verdict["wbits+empty/plain/host"] == "ok"
    assert verdict["wbits+empty/dict/device"] == "wbits" and verdict["wbits+empty/dict/host"] == "ok"
    # ... and only the host _dict entry wants its arrays even then
    assert verdict["dict_arrays+empty/dict/device"] == "ok" and verdict["dict_arrays+empty/dict/host"] == "dict_arrays"
    assert verdict["wbits+dict_arrays+empty/dict/device"] == "wbits"
    assert verdict["wbits+dict_arrays+empty/dict/host"] == "dict_arrays"
    # ... the host _dict entry names a dictionary's fault before windowBits, the device entry after it
    assert verdict["wbits+dict_arrays/dict/device"] == "wbits" and verdict["wbits+dict_arrays/dict/host"] == "dict_arrays"
    assert verdict["wbits+dict_buffer/dict/device"] == "wbits" and verdict["wbits+dict_buffer/dict/host"] == "dict_buffer"
    # ... the arrays before the buffer before the format, for both
    for where in ("device", "host"):
        assert verdict["dict_arrays+dict_buffer/dict/" + where] == "dict_arrays"
        assert verdict["gzip+dict_buffer/dict/" + where] == "dict_buffer"
        assert verdict["gzip/dict/" + where] == verdict["d64/dict/" + where] == "dict_format"
        # (lengths of 0 are the plain batch: no buffer is wanted, gzip is fine)
        assert verdict["gzip+dict_buffer+lens0/dict/" + where] == "ok"
        assert verdict["gzip+dict_buffer/plain/" + where] == "ok"
        assert verdict["null_ctx+wbits/dict/" + where] == verdict["null_ctx+dict_arrays+empty/dict/" + where] == "null_context"
    # ... alignment last, and the device entries' alone (the host entries stage their own regions)
    assert verdict["gzip+align_off/dict/device"] == "dict_format" and verdict["align_off/plain/device"] == "align"
    assert verdict["align_cap/dict/device"] == "align" and verdict["align_off+align_cap/plain/host"] == "ok"
    assert verdict["align_off+empty/plain/device"] == "ok"


def test_the_emulator_is_clean_under_asan_and_ubsan(build):
    exe, r = build("emu_plan_inflate_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        # only the linker missing a runtime library is "absent"; any other failure of the build is one
        if re.search(r"cannot find -l(asan|ubsan)|lib(asan|ubsan)[\w.]*: (cannot open|No such file)", r.stderr):
            pytest.skip("no sanitizer runtime")
        raise AssertionError(r.stderr)
    assert run(exe) == fc.emu_expected()


def real_call(L, kind, a, handle, mem=None):
    """the row through the real entry of its kind.  mem: the call's memory (test_gpu_inflate_faults.py);
    without it, whatever: an entry without a context reads none of it."""
    n = a["n"]
    u32, u64 = ctypes.c_uint32 * max(1, n), ctypes.c_uint64 * max(1, n)
    m = mem or {}
    res = m.get("res") or [(ctypes.c_int32 * max(1, n))() for _ in range(3)] + [u32() for _ in range(3)]
    device = kind.endswith("device")
    ioffs, ilens = u64(*m.get("in_off", [0] * n)), u32(*m.get("in_len", [0] * n))
    head = [handle, a["wbits"], n, m.get("in", None if device else b""), ioffs, ilens, m.get("out"), u64(*a["offs"]),
            u32(*a["caps"])]
    tail = []
    if kind.startswith("dict"):
        tail = [m.get("dict") if a["buf"] else None, u64(*m.get("dict_off", [0] * n)) if a["arrays"] else None,
                u32(*a["lens"]) if a["arrays"] else None]
    if kind == "device":
        return L.zs_inflate_batch_device(*head, *res[:5], None)
    if kind == "dict_device":
        return L.zs_inflate_batch_dict_device(*head, *res, None, *tail)
    return (L.zs_inflate_batch_dict if tail else L.zs_inflate_batch_ex)(*head, *res, *tail)


def test_rows_without_a_context_through_the_real_entries():
    import zsamd

    L = zsamd.lib()
    rows = [r for r in fc.rows() if "null_ctx" in r]
    assert len(rows) >= 2 * len(fc.FAULTS)
    for row in rows:
        for kind in fc.KINDS:
            assert fc.expected(kind, row) == "null_context"
            assert L.zs_set_option(None, b"timing", 0) != 0  # (another message in between)
            assert L.zs_last_error() == b"invalid arguments"
            rc = real_call(L, kind, fc.arguments(row), None)
            assert (rc, L.zs_last_error().decode()) == (fc.ZS_STREAM_ERROR, fc.MESSAGES["null_context"]), (row, kind)
